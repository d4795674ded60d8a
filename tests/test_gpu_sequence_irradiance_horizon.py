"""Irradiance of frame sequences under a horizon profile on the GPU
(sunsky_sequence_irradiance_horizon): the kernel per lane against its definition over the read-back
tables (tests/sequence_irradiance_horizon_reference.py) for every loop shape, shared and
per-receiver profiles, the exact cases (open, closed, boundaries, NaN), every launch shape, the
grid, the two code objects, graph capture, and what a uniform horizon means."""
import ctypes as C
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import sunsky_amd as ss
import gpu_sequence_irradiance_horizon_worker as W
from sunsky_amd import _capi
from sequence_irradiance_horizon_reference import HorizonReference
from test_gpu_sequence_irradiance import LAMBDAS_32, N_ALL, full_batch, host, local_of

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
# (table, sectors): sector lengths 20, 5 (a remainder of the 4-cell unroll), 1 (no inner loop), 8, 1, 4, 8
SHAPES = [((3, 20), 1), ((3, 20), 4), ((3, 20), 20), ((8, 16), 2), ((8, 16), 16), ((16, 32), 8), ((64, 256), 32)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def reference(variant, rotated, frames="five", size=(16, 32), lam=None):
    return HorizonReference(full_batch(variant, rotated, frames, size, lam).c.seq)


@functools.lru_cache(maxsize=None)
def horizon_batch(variant, rotated, frames="five", size=(16, 32), lam=None, sectors=8):
    """The forward test's 4,099 normals under 4,099 random profiles, and under the first of them
    shared: computed once and shared (read only)."""
    b = full_batch(variant, rotated, frames, size, lam)
    h = W.profiles(sectors, N_ALL, 1000 + sectors)
    nrm, hd = dev(b.n), dev(h)
    return types.SimpleNamespace(b=b, c=b.c, n=b.n, h=h, ref=reference(variant, rotated, frames, size, lam),
                                 E=host(b.c.seq.irradiance(nrm, horizon=hd)),
                                 E_shared=host(b.c.seq.irradiance(nrm, horizon=hd[:, 0].contiguous())))


def check_against_reference(ref, c, n_world, h, E, what):
    sky, sun, A, partial = ref.parts(local_of(n_world, c.tw), h)
    err, bound = np.abs(E.astype(np.float64) - (sky + sun)), ref.bound(A, partial)
    ratio = err / np.maximum(bound, 1e-300)
    print(f"{what}: worst {ratio.max():.3f} x bound, sun part up to "
          f"{np.abs(sun).max() / max(np.abs(sky + sun).max(), 1e-300):.2f} of E")
    assert np.all(np.isfinite(E)) and np.all(err <= bound), (what, float(ratio.max()), int((err > bound).sum()))
    return sky, sun


# ---------------------------------------------------------------- 1. the kernel against its definition
CASES = ([(v, r, "five", s, None, H) for v in VARIANTS for r in (False, True) for s, H in SHAPES] +
         [(v, r, f, (16, 32), None, 8) for v in VARIANTS for r in (False, True) for f in ("day", "one")] +
         [("spectral", r, "five", s, lam, H) for r in (False, True) for s, H in (((3, 20), 4), ((16, 32), 8))
          for lam in ((550.0,), tuple(LAMBDAS_32))])


@pytest.mark.parametrize("variant,rotated,frames,size,lam,sectors", CASES)
def test_horizon_irradiance_per_lane_against_the_definition(variant, rotated, frames, size, lam, sectors):
    """E of every one of the 4,099 lanes, under per-receiver profiles uniform in [-0.2, 1.2] (rows
    cut mid-cell, sectors fully open and fully closed) and under one shared profile, against the
    fp64 restatement within HorizonReference.bound (derived there).  A shared profile gives the
    bits of the same profile repeated per receiver.  No lane is left out."""
    hb = horizon_batch(variant, rotated, frames, size, lam, sectors)
    c = hb.c
    planes = 3 if variant == "rgb" else len(c.lam)
    what = f"{variant} rotated={rotated} {frames} {size} H={sectors} P={planes}"
    assert hb.E.shape == (planes, N_ALL) == hb.E_shared.shape
    sky, sun = check_against_reference(hb.ref, c, hb.n, hb.h, hb.E, what + " per receiver")
    check_against_reference(hb.ref, c, hb.n, hb.h[:, 0], hb.E_shared, what + " shared")
    assert np.abs(hb.E).max() > 0 and np.any(hb.E != hb.b.E)
    if frames != "one":
        assert np.abs(sun).max() > 0   # some receiver sees a sun
    repeated = dev(np.repeat(hb.h[:, :1], N_ALL, axis=1))
    np.testing.assert_array_equal(host(c.seq.irradiance(dev(hb.n), horizon=repeated)), hb.E_shared)
    column = dev(hb.h[:, :1])          # the (H, 1) form of a shared profile
    np.testing.assert_array_equal(host(c.seq.irradiance(dev(hb.n), horizon=column)), hb.E_shared)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_horizons_on_row_boundaries_and_on_a_suns_height(variant, rotated):
    """h exactly on the row boundaries i0 / n_z (v is exactly 0 or 1 everywhere) and, in the
    sectors of the two high suns, exactly the sun's z for some receivers and the next float above
    it for the others: equality counts as visible, the next float hides the sun."""
    b = full_batch(variant, rotated)
    ref = reference(variant, rotated)
    r = np.arange(N_ALL)
    h = np.stack([((r + 3 * s) % 17) / 16.0 for s in range(8)]).astype(np.float32)
    cols = b.c.seq.irradiance_sun_columns()
    assert list(cols // 4) == [0, 2, 4, 6, 0]
    z = np.array([b.c.seq.frame(k)["sun_dir_local"][2] for k in range(5)], np.float32)
    for k, sector, period in ((1, 2, 3), (3, 6, 2)):
        h[sector] = np.where(r % period == 0, z[k], np.nextafter(z[k], np.float32(2.0)))
    E = host(b.c.seq.irradiance(dev(b.n), horizon=dev(h)))
    check_against_reference(ref, b.c, b.n, h, E, f"{variant} rotated={rotated} boundaries")
    # explicitly: two receivers facing local up, all sectors at frame 1's z / the next float
    up = np.asarray(b.c.tw, np.float64)[:3, 2] if rotated else np.array([0.0, 0.0, 1.0])
    two = np.repeat(up[:, None], 2, axis=1).astype(np.float32)
    hh = np.repeat(np.array([[z[1], np.nextafter(z[1], np.float32(2.0))]], np.float32), 8, axis=0)
    e = host(b.c.seq.irradiance(dev(two), horizon=dev(hh))).astype(np.float64)
    term = ref.sun_terms[:, 1] * float(z[1])
    lit = np.abs(term) > 0
    assert lit.any() and np.all(np.abs((e[:, 0] - e[:, 1]) - term)[lit] <= 1e-3 * np.abs(term)[lit] + 1e-5 * np.abs(e[:, 0])[lit])


# ---------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_open_and_closed_horizons_are_exact(variant, rotated):
    """h = 0, h = -1 and a shared zero profile give irradiance() bit for bit; h = 2 gives exact zeros."""
    b = full_batch(variant, rotated)
    seq, nrm = b.c.seq, dev(b.n)
    for sectors in (1, 8, 32):
        for value in (0.0, -0.0, -1.0):
            per = torch.full((sectors, N_ALL), value, device="cuda")
            np.testing.assert_array_equal(host(seq.irradiance(nrm, horizon=per)), b.E)
        np.testing.assert_array_equal(host(seq.irradiance(nrm, horizon=torch.zeros(sectors, device="cuda"))), b.E)
        np.testing.assert_array_equal(host(seq.irradiance(nrm, horizon=torch.full((sectors, 1), -1.0, device="cuda"))), b.E)
        for closed in (torch.full((sectors, N_ALL), 2.0, device="cuda"), torch.full((sectors,), 2.0, device="cuda"),
                       torch.full((sectors,), float(np.nextafter(np.float32(1), np.float32(2))), device="cuda")):
            out = torch.full(b.E.shape, 7.0, device="cuda")
            seq.irradiance(nrm, horizon=closed, out=out)
            assert np.all(host(out) == 0)
    assert np.abs(b.E).max() > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_nan_profile_touches_its_receiver_only(variant):
    """Receivers with a NaN in their profile (all sectors, or one) are unspecified; every other
    receiver keeps its bits, the one that shares a lane with a NaN receiver included."""
    hb = horizon_batch(variant, False)
    bad = [0, 5, 2049, 2050, N_ALL - 1]   # 2049 / 2050: either side of the lane pairing (t, t + 2050)
    h = hb.h.copy()
    h[:, bad] = np.nan
    h[3, 77] = np.nan
    E = host(hb.c.seq.irradiance(dev(hb.n), horizon=dev(h)))
    keep = np.setdiff1d(np.arange(N_ALL), bad + [77])
    np.testing.assert_array_equal(E[:, keep], hb.E[:, keep])


# ---------------------------------------------------------------- 3. launch shapes
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_launch_shapes_are_bitwise_the_full_batch(variant, rotated):
    """Empty batches, 1-7 lanes from unaligned planes, a mask, a row-strided out, a row-strided
    horizon and a second run give, bit for bit, the values those lanes have inside the 4,099-lane batch."""
    hb = horizon_batch(variant, rotated)
    seq, P, H = hb.c.seq, hb.E.shape[0], hb.h.shape[0]
    nrm, hd = dev(hb.n), dev(hb.h)
    np.testing.assert_array_equal(host(seq.irradiance(nrm, horizon=hd)), hb.E)   # two runs
    e = host(seq.irradiance(nrm[:, :0], horizon=hd[:, :0]))
    assert e.shape == (P, 0) and host(seq.irradiance(nrm[:, :0], horizon=hd[:, 0].contiguous())).shape == (P, 0)
    assert ss.lib().sunsky_sequence_irradiance_horizon(seq._h, _capi.Vec3In(None, None, None), None, 0, 0, 0, None, 0, None,
                                                       0, None) == 0
    for n in range(1, 8):
        for lo in (0, 1, 4092):
            flat = torch.empty(3 * n + 1, device="cuda")   # planes 4 bytes off any 16-byte boundary
            nn = flat[1:].view(3, n)
            nn.copy_(nrm[:, lo:lo + n])
            hflat = torch.empty(H * n + 1, device="cuda")
            hh = hflat[1:].view(H, n)
            hh.copy_(hd[:, lo:lo + n])
            assert nn.data_ptr() % 16 == 4 and hh.data_ptr() % 16 == 4
            oflat = torch.full((P * n + 1,), 7.0, device="cuda")
            out = oflat[1:].view(P, n)
            assert seq.irradiance(nn, out=out, horizon=hh) is out
            np.testing.assert_array_equal(host(out), hb.E[:, lo:lo + n])
            assert float(oflat[0]) == 7.0
            sflat = torch.empty(H + 1, device="cuda")             # a shared profile from an unaligned plane
            sflat[1:].copy_(hd[:, lo])
            seq.irradiance(nn, out=out, horizon=sflat[1:])
            np.testing.assert_array_equal(host(out), host(seq.irradiance(nn, horizon=hd[:, lo].contiguous())))
    mask = dev((np.arange(N_ALL) % 2).astype(np.uint8))
    m = host(seq.irradiance(nrm, active=mask, horizon=hd))
    assert np.all(m[:, ::2] == 0) and np.any(hb.E[:, ::2] != 0)
    np.testing.assert_array_equal(m[:, 1::2], hb.E[:, 1::2])
    wide = torch.full((P, N_ALL + 13), 7.0, device="cuda")   # a row stride larger than n
    out = wide[:, :N_ALL]
    assert out.stride(0) == N_ALL + 13 and seq.irradiance(nrm, out=out, horizon=hd) is out
    np.testing.assert_array_equal(host(out), hb.E)
    assert np.all(host(wide[:, N_ALL:]) == 7.0)
    hwide = torch.full((H, N_ALL + 29), float("nan"), device="cuda")   # the same for the horizon
    hs = hwide[:, :N_ALL]
    hs.copy_(hd)
    assert hs.stride(0) == N_ALL + 29
    np.testing.assert_array_equal(host(seq.irradiance(nrm, horizon=hs)), hb.E)
    shared_strided = hwide[:, 5]                                         # a shared profile, sectors N_ALL + 29 apart
    np.testing.assert_array_equal(host(seq.irradiance(nrm, horizon=shared_strided)),
                                  host(seq.irradiance(nrm, horizon=hd[:, 5].contiguous())))
    np.testing.assert_array_equal(host(seq.irradiance(nrm, horizon=hd.t().contiguous().t())), hb.E)   # columns contiguous: copied
    v3 = _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)])
    L = ss.lib()
    assert L.sunsky_sequence_irradiance_horizon(seq._h, v3, hd.data_ptr(), H, N_ALL, N_ALL - 1, None, N_ALL, wide.data_ptr(),
                                                N_ALL + 13, None) == 1
    assert b"horizon_stride" in L.sunsky_last_error()
    assert L.sunsky_sequence_irradiance_horizon(seq._h, v3, hd.data_ptr(), H, N_ALL, N_ALL, None, N_ALL, wide.data_ptr(),
                                                N_ALL - 1, None) == 1
    assert b"out_stride" in L.sunsky_last_error()
    assert L.sunsky_sequence_irradiance_horizon(seq._h, v3, hd.data_ptr(), 5, N_ALL, N_ALL, None, N_ALL, wide.data_ptr(),
                                                N_ALL + 13, None) == 1
    assert b"n_sectors" in L.sunsky_last_error()
    with pytest.raises(ValueError, match="horizon must be on"):
        seq.irradiance(nrm, horizon=torch.zeros(H))


# ---------------------------------------------------------------- 4. grid
def test_a_grid_smaller_than_the_work_is_bitwise_the_default_grid(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 walks the grid-stride loop two to three
    times per lane; this process makes the same calls at the default grid (one step)."""
    n = W.batch_size()
    env = dict(os.environ, SUNSKY_AMD_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, W.__file__, str(n), str(tmp_path)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    for variant in W.VARIANTS:
        child, mine = np.load(tmp_path / f"{variant}.npy"), W.run(variant, n)
        assert child.shape == mine.shape and np.any(mine[0] != 0) and np.any(mine[1] != 0)
        np.testing.assert_array_equal(child, mine)


# ---------------------------------------------------------------- 5. code objects
@pytest.mark.parametrize("variant", VARIANTS)
def test_identity_code_object_gives_the_general_ones_bits(variant, monkeypatch):
    hb = horizon_batch(variant, False)
    monkeypatch.setenv("SUNSKY_AMD_GENERAL_XFORM", "1")
    np.testing.assert_array_equal(host(hb.c.seq.irradiance(dev(hb.n), horizon=dev(hb.h))), hb.E)
    np.testing.assert_array_equal(host(hb.c.seq.irradiance(dev(hb.n), horizon=dev(hb.h[:, 0]))), hb.E_shared)


# ---------------------------------------------------------------- 6. graph capture
@pytest.mark.parametrize("variant", VARIANTS)
def test_horizon_irradiance_replays_bitwise_from_a_graph(variant):
    """Captured once on a side stream and replayed twice: the output equals the direct call bit
    for bit; nothing is allocated between capture and replay."""
    hb = horizon_batch(variant, False)
    L, P, H = ss.lib(), hb.E.shape[0], hb.h.shape[0]
    nrm, hd = dev(hb.n), dev(hb.h)
    out = torch.zeros((P, N_ALL), device="cuda")

    def call():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.sunsky_sequence_irradiance_horizon(hb.c.seq._h, _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)]),
                                                    hd.data_ptr(), H, N_ALL, N_ALL, None, N_ALL, out.data_ptr(), N_ALL, st) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    allocated = torch.cuda.memory_allocated()
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), hb.E)
    assert torch.cuda.memory_allocated() == allocated


# ---------------------------------------------------------------- 7. what a uniform horizon means
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("i0", [5, 6])
def test_a_uniform_horizon_on_a_row_boundary_removes_the_rows_below_it(variant, i0):
    """K = 1 (a 20 degree sun, z = 0.342), 16 x 32 cells, one shared horizon h = i0 / 16: E is the
    unoccluded restatement (tests/sequence_irradiance_reference.py) with the rows below i0 removed
    and the sun kept at i0 = 5 (h = 0.3125) and dropped at i0 = 6 (h = 0.375)."""
    b = full_batch(variant, False, "one")
    r = reference(variant, False, "one")
    h = np.full(8, i0 / 16.0, np.float32)
    E = host(b.c.seq.irradiance(dev(b.n), horizon=dev(h))).astype(np.float64)
    terms = r.sky_terms.reshape(r.planes, 16, 32).copy()
    terms[:, :i0] = 0
    terms = terms.reshape(r.planes, -1)
    nl = local_of(b.n, None)
    cos = np.maximum(nl @ r.centres.T, 0.0)
    seen = 1.0 if i0 == 5 else 0.0
    cos_sun = np.maximum(nl @ r.suns.T, 0.0) * seen
    want = terms @ cos.T + r.sun_terms @ cos_sun.T
    A = np.abs(terms) @ cos.T + np.abs(r.sun_terms) @ cos_sun.T
    err, bound = np.abs(E - want), r.bound(A, np.zeros_like(A))
    print(f"{variant} i0={i0}: worst {np.max(err / np.maximum(bound, 1e-300)):.3f} x bound")
    assert np.all(err <= bound) and np.abs(r.sun_terms).max() > 0 and np.abs(E).max() > 0
    assert (np.abs(E - b.E).max() > 0)
