"""The per-frame irradiance series on the GPU (sunsky_sequence_prepare_irradiance_series /
_irradiance_series): every frame's planes bit for bit against irradiance() and
irradiance(horizon=) of the one-frame, weight-1 sequence, per lane against the definition over
the read-back tables (tests/sequence_irradiance_series_reference.py), the weighted sum against
irradiance(), frame groups and sub-ranges, every launch shape, the grid, the two code objects,
graph capture and the device frame tables."""
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
import gpu_sequence_irradiance_series_worker as W
from gpu_sequence_irradiance_horizon_worker import profiles
from sunsky_amd import _capi
from sequence_irradiance_series_reference import SeriesReference
from test_gpu_sequence_irradiance import EPS, LAMBDAS_32, N_ALL, full_batch, host, local_of
from test_gpu_sequence_irradiance_horizon import SHAPES

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
TABLES = [(3, 20), (8, 16), (16, 32)]
LAMS = [(550.0,), tuple(LAMBDAS_32)]          # P = 1: the widest group (G = 8); P = 32: G = 1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def series_batch(variant, rotated, frames="five", size=(16, 32), lam=None):
    """The forward test's sequence with the series prepared, and its series over the forward
    test's 4,099 normals: computed once and shared (read only)."""
    b = full_batch(variant, rotated, frames, size, lam)
    seq = b.c.seq
    seq.prepare_irradiance_series()
    S = host(seq.irradiance_series(dev(b.n)))
    planes = 3 if variant == "rgb" else len(b.c.lam)
    assert S.shape == (b.c.K, planes, N_ALL) and S.dtype == np.float32
    return types.SimpleNamespace(b=b, c=b.c, seq=seq, n=b.n, S=S, K=b.c.K, P=planes, G=_capi.seq_irr_series_group(planes))


@functools.lru_cache(maxsize=None)
def horizon_series(variant, rotated, frames="five", size=(16, 32), lam=None, sectors=8):
    """... and under 4,099 per-receiver profiles, and under the first of them shared."""
    sb = series_batch(variant, rotated, frames, size, lam)
    h = profiles(sectors, N_ALL, 1000 + sectors)
    nrm, hd = dev(sb.n), dev(h)
    return types.SimpleNamespace(sb=sb, h=h, S=host(sb.seq.irradiance_series(nrm, horizon=hd)),
                                 S_shared=host(sb.seq.irradiance_series(nrm, horizon=hd[:, 0].contiguous())))


@functools.lru_cache(maxsize=None)
def reference(variant, rotated, frames="five", size=(16, 32), lam=None):
    return SeriesReference(series_batch(variant, rotated, frames, size, lam).seq)


def one_frame(c, k, size):
    """The sequence that holds frame k alone with weight 1, on the same grid and wavelength list."""
    one = ss.SunskySequence(c.parent, c.dirs[k:k + 1], c.turb[k:k + 1], [1.0])
    one.prepare_irradiance(*size, wavelengths=c.lam)
    return one


def night_frames(c):
    return [k for k in range(c.K) if c.seq.frame(k)["sun_dir_local"][2] < 0]


def check_against_reference(ref, c, n_world, S, what, h=None):
    sky, sun, A, partial = ref.parts(local_of(n_world, c.tw), h)
    err = np.abs(S.astype(np.float64) - (sky + sun))
    bound = ref.bound(A, None if h is None else partial)
    ratio = err / np.maximum(bound, 1e-300)
    print(f"{what}: worst {ratio.max():.3f} x bound, sun part up to "
          f"{np.abs(sun).max() / max(np.abs(sky + sun).max(), 1e-300):.2f} of E")
    assert np.all(np.isfinite(S)) and np.all(err <= bound), (what, float(ratio.max()), int((err > bound).sum()))


# ---------------------------------------------------------------- 1. one-frame sequences and the definition
OPEN_CASES = ([(v, r, "five", s, None) for v in VARIANTS for r in (False, True) for s in TABLES] +
              [(v, False, "five", (64, 256), None) for v in VARIANTS] +
              [(v, r, f, (16, 32), None) for v in VARIANTS for r in (False, True) for f in ("day", "one")] +
              [("spectral", r, "five", s, lam) for r in (False, True) for s in ((3, 20), (16, 32)) for lam in LAMS])


@pytest.mark.parametrize("variant,rotated,frames,size,lam", OPEN_CASES)
def test_every_frame_is_bitwise_its_one_frame_sequence(variant, rotated, frames, size, lam):
    """Planes [k P, (k + 1) P) of the series equal irradiance() of the sequence that holds frame k
    alone with weight 1, for every frame and all 4,099 lanes; night frames are exact zeros, the
    zero-weight frame has its weight-1 value; every lane within the bound of the fp64 definition."""
    sb = series_batch(variant, rotated, frames, size, lam)
    nrm = dev(sb.n)
    for k in range(sb.K):
        E = host(one_frame(sb.c, k, size).irradiance(nrm))
        assert sb.S[k].tobytes() == E.tobytes(), (variant, rotated, frames, size, k, int((sb.S[k] != E).sum()))
    night = night_frames(sb.c)
    for k in night:
        assert np.all(sb.S[k] == 0), k
    if frames != "one":
        assert night and len(night) < sb.K
        dark = [k for k in range(sb.K) if sb.c.wts[k] == 0]
        assert dark and all(k not in night and np.abs(sb.S[k]).max() > 0 for k in dark)
    assert np.abs(sb.S).max() > 0
    check_against_reference(reference(variant, rotated, frames, size, lam), sb.c, sb.n, sb.S,
                            f"{variant} rotated={rotated} {frames} {size} P={sb.P}")


HORIZON_CASES = ([(v, r, "five", s, None, H) for v in VARIANTS for r in (False, True) for s, H in SHAPES] +
                 [(v, r, f, (16, 32), None, 8) for v in VARIANTS for r in (False, True) for f in ("day", "one")] +
                 [("spectral", False, "five", (16, 32), lam, 8) for lam in LAMS])


@pytest.mark.parametrize("variant,rotated,frames,size,lam,sectors", HORIZON_CASES)
def test_every_frame_is_bitwise_its_one_frame_sequence_under_a_horizon(variant, rotated, frames, size, lam, sectors):
    """The same under per-receiver profiles uniform in [-0.2, 1.2] and under one shared profile,
    against irradiance(horizon=) of the one-frame sequences and against the fp64 definition."""
    hs = horizon_series(variant, rotated, frames, size, lam, sectors)
    sb = hs.sb
    nrm, hd = dev(sb.n), dev(hs.h)
    shared = hd[:, 0].contiguous()
    for k in range(sb.K):
        one = one_frame(sb.c, k, size)
        E = host(one.irradiance(nrm, horizon=hd))
        assert hs.S[k].tobytes() == E.tobytes(), (variant, rotated, frames, size, sectors, k, int((hs.S[k] != E).sum()))
        E = host(one.irradiance(nrm, horizon=shared))
        assert hs.S_shared[k].tobytes() == E.tobytes(), (variant, rotated, frames, size, sectors, k, "shared")
    for k in night_frames(sb.c):
        assert np.all(hs.S[k] == 0) and np.all(hs.S_shared[k] == 0), k
    assert np.abs(hs.S).max() > 0 and np.any(hs.S != sb.S)
    ref = reference(variant, rotated, frames, size, lam)
    what = f"{variant} rotated={rotated} {frames} {size} H={sectors} P={sb.P}"
    check_against_reference(ref, sb.c, sb.n, hs.S, what + " per receiver", hs.h)
    check_against_reference(ref, sb.c, sb.n, hs.S_shared, what + " shared", hs.h[:, 0])
    # the (H, 1) form of a shared profile
    np.testing.assert_array_equal(host(sb.seq.irradiance_series(nrm, horizon=dev(hs.h[:, :1]))), hs.S_shared)


# ---------------------------------------------------------------- 2. consistency with the weighted sum
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("frames", ["five", "day", "one"])
def test_the_weighted_sum_of_the_series_is_the_irradiance(variant, rotated, frames):
    """sum_k w_k series_k (fp64) against irradiance() of the weighted sequence: the tables of the
    latter are the frame-order fp32 accumulation of the former's (K roundings, then omega and the
    weight: K + 2), on top of the forward's own bound."""
    sb = series_batch(variant, rotated, frames)
    w = np.asarray(sb.c.wts, np.float32).astype(np.float64)[:, None, None]
    S = sb.S.astype(np.float64)
    total, mag = (w * S).sum(0), (np.abs(w) * np.abs(S)).sum(0)
    _, _, A = sb.c.ref.parts(local_of(sb.n, sb.c.tw))
    bound = (sb.K + 2) * EPS * mag + sb.c.ref.bound(A)
    err = np.abs(sb.b.E.astype(np.float64) - total)
    print(f"{variant} rotated={rotated} {frames}: worst {np.max(err / np.maximum(bound, 1e-300)):.3f} x bound")
    assert np.all(err <= bound) and np.abs(total).max() > 0


# ---------------------------------------------------------------- 3. groups and ranges
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_frame_ranges_are_bitwise_slices_of_the_full_call(variant, rotated):
    """frames=(f, c) over the day's 24 frames, for f and c on, before and behind the group
    boundaries: bit for bit the slice of the full call, with an open horizon and under profiles."""
    sb = series_batch(variant, rotated, "day")
    hs = horizon_series(variant, rotated, "day")
    G, nrm, hd = sb.G, dev(sb.n), dev(hs.h)
    assert sb.K == 24 and G == (8 if variant == "rgb" else 4)
    seen = 0
    for f in (0, 1, G - 1, G, 23):
        for c in (0, 1, G, G + 1, 24 - f):
            if f + c > 24:
                continue
            got = host(sb.seq.irradiance_series(nrm, frames=(f, c)))
            assert got.shape == (c, sb.P, N_ALL)
            np.testing.assert_array_equal(got, sb.S[f:f + c])
            got = host(sb.seq.irradiance_series(nrm, frames=range(f, f + c), horizon=hd))
            np.testing.assert_array_equal(got, hs.S[f:f + c])
            seen += 1
    assert seen >= 20


# ---------------------------------------------------------------- 4. launch shapes
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_launch_shapes_are_bitwise_the_full_batch(variant, rotated):
    """Empty batches, 1-7 lanes from unaligned planes, a mask, a row-strided out, a row-strided
    horizon and a second run give, bit for bit, the values those lanes have inside the 4,099-lane batch."""
    hs = horizon_series(variant, rotated)
    sb = hs.sb
    seq, K, P, H = sb.seq, sb.K, sb.P, hs.h.shape[0]
    nrm, hd = dev(sb.n), dev(hs.h)
    np.testing.assert_array_equal(host(seq.irradiance_series(nrm)), sb.S)                  # two runs
    np.testing.assert_array_equal(host(seq.irradiance_series(nrm, horizon=hd)), hs.S)
    assert host(seq.irradiance_series(nrm[:, :0])).shape == (K, P, 0)
    assert host(seq.irradiance_series(nrm[:, :0], horizon=hd[:, :0])).shape == (K, P, 0)
    assert host(seq.irradiance_series(nrm, frames=(2, 0))).shape == (0, P, N_ALL)
    L = ss.lib()
    none3 = _capi.Vec3In(None, None, None)
    assert L.sunsky_sequence_irradiance_series(seq._h, none3, None, 0, 0, 0, None, 0, 0, K, None, 0, None) == 0
    assert L.sunsky_sequence_irradiance_series(seq._h, none3, None, 0, 0, 0, None, N_ALL, 0, 0, None, 0, None) == 0
    for n in range(1, 8):
        for lo in (0, 1, 4092):
            flat = torch.empty(3 * n + 1, device="cuda")   # planes 4 bytes off any 16-byte boundary
            nn = flat[1:].view(3, n)
            nn.copy_(nrm[:, lo:lo + n])
            hflat = torch.empty(H * n + 1, device="cuda")
            hh = hflat[1:].view(H, n)
            hh.copy_(hd[:, lo:lo + n])
            assert nn.data_ptr() % 16 == 4 and hh.data_ptr() % 16 == 4
            oflat = torch.full((K * P * n + 1,), 7.0, device="cuda")
            out = oflat[1:].view(K, P, n)
            assert seq.irradiance_series(nn, out=out) is out
            np.testing.assert_array_equal(host(out), sb.S[:, :, lo:lo + n])
            assert seq.irradiance_series(nn, out=out, horizon=hh) is out
            np.testing.assert_array_equal(host(out), hs.S[:, :, lo:lo + n])
            assert float(oflat[0]) == 7.0
            sflat = torch.empty(H + 1, device="cuda")             # a shared profile from an unaligned plane
            sflat[1:].copy_(hd[:, 0])
            seq.irradiance_series(nn, out=out, horizon=sflat[1:])
            np.testing.assert_array_equal(host(out), hs.S_shared[:, :, lo:lo + n])
    mask = dev((np.arange(N_ALL) % 2).astype(np.uint8))
    for S, kw in ((sb.S, {}), (hs.S, {"horizon": hd})):
        m = host(seq.irradiance_series(nrm, active=mask, **kw))
        assert np.all(m[:, :, ::2] == 0) and np.any(S[:, :, ::2] != 0)
        np.testing.assert_array_equal(m[:, :, 1::2], S[:, :, 1::2])
    wide = torch.full((K, P, N_ALL + 13), 7.0, device="cuda")   # a row stride larger than n
    out = wide[:, :, :N_ALL]
    assert out.stride(1) == N_ALL + 13 and seq.irradiance_series(nrm, out=out) is out
    np.testing.assert_array_equal(host(out), sb.S)
    assert np.all(host(wide[:, :, N_ALL:]) == 7.0)
    part = wide[:3, :, :N_ALL]                                   # ... for a sub-range of the frames
    wide.fill_(7.0)
    assert seq.irradiance_series(nrm, frames=(1, 3), out=part, horizon=hd) is part
    np.testing.assert_array_equal(host(part), hs.S[1:4])
    assert np.all(host(wide[:, :, N_ALL:]) == 7.0) and np.all(host(wide[3:]) == 7.0)
    hwide = torch.full((H, N_ALL + 29), float("nan"), device="cuda")   # the same for the horizon
    hstr = hwide[:, :N_ALL]
    hstr.copy_(hd)
    assert hstr.stride(0) == N_ALL + 29
    np.testing.assert_array_equal(host(seq.irradiance_series(nrm, horizon=hstr)), hs.S)
    with pytest.raises(ValueError, match="out must be a float32 tensor of shape"):
        seq.irradiance_series(nrm, out=torch.empty((K, P, N_ALL - 1), device="cuda"))
    with pytest.raises(ValueError, match="out planes must be contiguous"):
        seq.irradiance_series(nrm, out=torch.empty((K, N_ALL, P), device="cuda").transpose(1, 2))
    v3 = _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)])
    assert L.sunsky_sequence_irradiance_series(seq._h, v3, None, 0, 0, 0, None, N_ALL, 0, K, wide.data_ptr(), N_ALL - 1,
                                               None) == 1
    assert b"out_stride" in L.sunsky_last_error()
    assert L.sunsky_sequence_irradiance_series(seq._h, v3, None, 0, 0, 0, None, N_ALL, 1, K, wide.data_ptr(), N_ALL + 13,
                                               None) == 1
    assert b"frame range" in L.sunsky_last_error()
    with pytest.raises(ValueError, match="horizon must be on"):
        seq.irradiance_series(nrm, horizon=torch.zeros(H))


def test_a_grid_smaller_than_the_work_is_bitwise_the_default_grid(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 walks the grid-stride loop over the work
    items (tile of receiver pairs, group) more than twice per workgroup; this process makes the
    same calls at the default grid (one step)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for variant in W.VARIANTS:
        assert W.work_items(W.frame_count(variant), 3 if variant == "rgb" else 32) > 2 * cus
    env = dict(os.environ, SUNSKY_AMD_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, W.__file__, str(tmp_path)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    for variant in W.VARIANTS:
        child, mine = np.load(tmp_path / f"{variant}.npy"), W.run(variant)
        assert child.shape == mine.shape and np.any(mine[0] != 0) and np.any(mine[1] != 0) and np.any(mine[0] != mine[1])
        assert child.tobytes() == mine.tobytes()


@pytest.mark.parametrize("variant", VARIANTS)
def test_identity_code_object_gives_the_general_ones_bits(variant, monkeypatch):
    hs = horizon_series(variant, False)
    monkeypatch.setenv("SUNSKY_AMD_GENERAL_XFORM", "1")
    np.testing.assert_array_equal(host(hs.sb.seq.irradiance_series(dev(hs.sb.n))), hs.sb.S)
    np.testing.assert_array_equal(host(hs.sb.seq.irradiance_series(dev(hs.sb.n), horizon=dev(hs.h))), hs.S)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("horizon", [False, True])
def test_the_series_replays_bitwise_from_a_graph(variant, horizon):
    """Captured once on a side stream and replayed twice: the output equals the direct call bit
    for bit; nothing is allocated between capture and replay."""
    hs = horizon_series(variant, False, "day")
    sb = hs.sb
    L, K, P, H = ss.lib(), sb.K, sb.P, hs.h.shape[0]
    nrm, hd = dev(sb.n), dev(hs.h)
    out = torch.zeros((K, P, N_ALL), device="cuda")
    want = hs.S if horizon else sb.S

    def call():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.sunsky_sequence_irradiance_series(sb.seq._h, _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)]),
                                                   hd.data_ptr() if horizon else None, H, N_ALL, N_ALL, None, N_ALL, 0, K,
                                                   out.data_ptr(), N_ALL, st) == 0

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
        np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert torch.cuda.memory_allocated() == allocated


# ---------------------------------------------------------------- 5. device tables
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("size", [(3, 20), (16, 32)])
def test_device_frame_tables_are_the_one_frame_sequences_device_tables(variant, rotated, size):
    """irradiance_frame_table(k) of a device sequence bit for bit the device "sky" table of the
    one-frame, weight-1 sequence, for all five frames; the night frame's and the 300 nm plane are 0."""
    c = full_batch(variant, rotated, "five", size).c
    for k in range(c.K):
        t = c.seq.irradiance_frame_table(k)
        want = one_frame(c, k, size).irradiance_table("sky")
        assert t.shape == want.shape and t.tobytes() == want.tobytes(), (variant, rotated, size, k)
        assert np.all(t == 0) if k == 4 else np.all(t[:3].max((1, 2)) > 0)
        if variant == "spectral":
            assert np.all(t[4] == 0)


def test_the_series_follows_new_tables_and_update():
    """Sticky on the device too: new tables restage the images, and after update() and new tables
    the series is that of a new sequence."""
    b = full_batch("rgb", False)
    c = b.c
    seq = ss.SunskySequence(c.parent, c.dirs, c.turb, c.wts)
    seq.prepare_irradiance(8, 16)
    seq.prepare_irradiance_series()
    seq.prepare_irradiance(16, 32)
    nrm = dev(b.n)
    np.testing.assert_array_equal(host(seq.irradiance_series(nrm)), series_batch("rgb", False).S)
    seq.update(sun_directions=c.dirs[::-1].copy(), turbidity=c.turb[::-1])
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):   # the tables went with it
        seq.irradiance_series(nrm)
    seq.prepare_irradiance(16, 32)
    np.testing.assert_array_equal(host(seq.irradiance_series(nrm)), series_batch("rgb", False).S[::-1])
