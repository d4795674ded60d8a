"""Irradiance of frame sequences on oriented receivers on the GPU (sunsky_sequence_prepare_irradiance /
_irradiance): the device tables, the kernel per lane against its definition over the read-back
tables (tests/sequence_irradiance_reference.py), every launch shape, the grid, the two code
objects, graph capture, and K = 1 end to end against the fp64 oracle's quadrature."""
import ctypes as C
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import oracle as O
import sunsky_amd as ss
import gpu_sequence_irradiance_worker as W
from sunsky_amd import _capi
from sequence_cases import (DAY_TIMES, DAY_TURBIDITY, DAY_WEIGHTS, LAMBDAS, TURBIDITY, WEIGHTS, base_dict, frame_dict,
                            frame_dirs, rotation, to_world_dirs)
from sequence_irradiance_reference import IrradianceReference
from sequence_sampling_reference import cell_centres
from test_direct_diffuse import WL, _cap_integral, quadrature

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
TABLES = [(8, 16), (16, 32), (64, 256), (3, 20)]   # (3, 20): no multiple of the kernel's 4-cell step
EPS = 2.0 ** -24
N_ALL = 4099
LAMBDAS_32 = [float(x) for x in np.linspace(330.0, 715.0, 31)] + [300.0]   # the last one is outside the model


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def local_of(n_world, tw):
    """(3, n) world vectors -> (n, 3) local, fp64 (R^-1 = R^T)."""
    d = np.asarray(n_world, np.float64).T
    return d if tw is None else d @ np.asarray(tw, np.float64)[:3, :3]


def frames_of(frames, parent, tw):
    if frames == "five":
        return frame_dirs(tw), TURBIDITY, WEIGHTS
    if frames == "day":
        m = np.asarray(parent.get_param("to_world"), np.float32)[:3, :3]
        return np.stack([m @ ss.sun_coordinates(*t) for t in DAY_TIMES]).astype(np.float32), DAY_TURBIDITY, DAY_WEIGHTS
    return frame_dirs(tw)[1:2], TURBIDITY[1:2], [1.0]   # K = 1


@functools.lru_cache(maxsize=None)
def sequence(variant, rotated, frames="five", size=(16, 32), lam=None):
    """A parent, its sequence with the irradiance tables prepared, and the numpy restatement."""
    tw = rotation() if rotated else None
    base = base_dict(**({"to_world": tw} if rotated else {}))
    parent = ss.SunskyEmitter(base, variant)
    dirs, turb, wts = frames_of(frames, parent, tw)
    seq = ss.SunskySequence(parent, dirs, turb, wts)
    lam = (list(lam) if lam else LAMBDAS) if variant == "spectral" else None
    seq.prepare_irradiance(*size, wavelengths=lam)
    return types.SimpleNamespace(base=base, tw=tw, parent=parent, seq=seq, ref=IrradianceReference(seq), dirs=dirs,
                                 turb=turb, wts=wts, K=len(turb), lam=lam, variant=variant)


def normals(c):
    """(3, 4099) fp32 world-space normals: uniform on the whole sphere, then +-z and +-x of the
    local frame, then 16 perpendicular to a frame's sun (4 about each of up to 4 suns above the
    horizon; exactly perpendicular in the local frame before the fp32 rounding of to_world)."""
    special = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0]]
    suns = [s for s in c.ref.suns if s[2] >= 0][:4]
    for i in range(16):
        s = suns[i % len(suns)]
        a = np.array([-s[1], s[0], 0.0])
        b = np.cross(s, a)
        t = 0.3 + 1.7 * (i // len(suns))
        special.append(np.cos(t) * a + np.sin(t) * b)
    local = np.concatenate([W.sphere_normals(N_ALL - len(special), 31).T.astype(np.float64), np.asarray(special)])
    if c.tw is None:
        return np.ascontiguousarray(local.T.astype(np.float32))
    return np.ascontiguousarray(to_world_dirs(local, c.tw).T)


@functools.lru_cache(maxsize=None)
def full_batch(variant, rotated, frames="five", size=(16, 32), lam=None):
    """irradiance over the 4,099 normals, computed once and shared (read only)."""
    c = sequence(variant, rotated, frames, size, lam)
    n = normals(c)
    return types.SimpleNamespace(c=c, n=n, E=host(c.seq.irradiance(torch.from_numpy(n).cuda())))


# ---------------------------------------------------------------- 1. device tables
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size", TABLES[:3])
def test_device_tables_match_the_host_tables_and_the_public_eval(variant, size):
    """Sky within 1e-5 of the host-only table's largest entry (per plane), flux rtol 1e-5; the sky
    table against sequence.eval of a sun_scale-0 sequence at the cell centres at the accumulation
    bar 1e-5 max|R_p| + (K + 2) 2^-24 |v| (the sky values are >= 0: the sum is the magnitude)."""
    c = sequence(variant, False, "five", size)
    R, F = c.seq.irradiance_table("sky").astype(np.float64), c.seq.irradiance_table("sun_flux")
    hs = ss.SunskySequence(ss.SunskyEmitter(c.base, variant, device="host"), c.dirs, c.turb, c.wts)
    hs.prepare_irradiance(*size, wavelengths=c.lam)
    Rh, Fh = hs.irradiance_table("sky").astype(np.float64), hs.irradiance_table("sun_flux")
    worst = (np.abs(R - Rh).max((1, 2)) / np.maximum(np.abs(Rh).max((1, 2)), 1e-300)).max()
    print(f"{variant} {size}: device vs host sky table {worst:.3e} of the largest entry")
    assert np.all(np.abs(R - Rh).max((1, 2)) <= 1e-5 * np.abs(Rh).max((1, 2)))
    np.testing.assert_allclose(F, Fh, rtol=1e-5, atol=0)
    assert np.any(F != 0) and np.all(F[:, 4] == 0)
    sky_parent = ss.SunskyEmitter(dict(c.base, sun_scale=0.0), variant, precision="reference")
    sky_seq = ss.SunskySequence(sky_parent, c.dirs, c.turb, c.wts)
    wi = torch.from_numpy(np.ascontiguousarray(-cell_centres(*size).T.astype(np.float32))).cuda()
    v = host(sky_seq.eval(wi, c.lam)).astype(np.float64)
    got = R.reshape(R.shape[0], -1)
    bound = 1e-5 * np.abs(got).max(1, keepdims=True) + (c.K + 2) * EPS * np.abs(v)
    err = np.abs(got - v)
    print(f"vs sequence.eval: worst {np.max(err / np.maximum(bound, 1e-300)):.3f} x bound")
    assert np.all(v >= 0) and np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
    if variant == "spectral":
        assert np.all(R[4] == 0) and np.all(F[4] == 0)


# ---------------------------------------------------------------- 2. the kernel against its definition
CASES = ([(v, r, "five", s, None) for v in VARIANTS for r in (False, True) for s in TABLES] +
         [(v, r, f, (16, 32), None) for v in VARIANTS for r in (False, True) for f in ("day", "one")] +
         [("spectral", r, "five", s, lam) for r in (False, True) for s in ((3, 20), (16, 32))
          for lam in ((550.0,), tuple(LAMBDAS_32))])


@pytest.mark.parametrize("variant,rotated,frames,size,lam", CASES)
def test_irradiance_per_lane_against_the_definition(variant, rotated, frames, size, lam):
    """E of every one of the 4,099 lanes against the fp64 sum over the read-back device tables:
    |E - E64| <= 1e-5 A + 8 2^-24 A' + (n_phi + n_z + K + 4) 2^-24 A per plane and receiver, with
    A = sum |terms| with the cosine and A' = sum omega |R| + sum w |F| without it (table rounding;
    rounding of the dot product and of to_local; accumulation depth).  No lane is left out."""
    b = full_batch(variant, rotated, frames, size, lam)
    c, r = b.c, b.c.ref
    planes = 3 if variant == "rgb" else len(c.lam)
    assert b.E.shape == (planes, N_ALL) and r.planes == planes and np.all(np.isfinite(b.E))
    sky, sun, A = r.parts(local_of(b.n, c.tw))
    err, bound = np.abs(b.E.astype(np.float64) - (sky + sun)), r.bound(A)
    ratio = err / np.maximum(bound, 1e-300)
    print(f"{variant} rotated={rotated} {frames} {size} P={planes}: worst {ratio.max():.3f} x bound, "
          f"sun part up to {np.abs(sun).max() / np.abs(sky + sun).max():.2f} of E")
    assert np.all(err <= bound), (float(ratio.max()), int((err > bound).sum()))
    assert np.abs(b.E).max() > 0 and np.abs(sun).max() > 0
    if not rotated:
        down = N_ALL - 20 + 1   # the normal (0, 0, -1)
        assert np.all(b.n[:, down] == [0, 0, -1]) and np.all(b.E[:, down] == 0)
    if variant == "spectral":
        bad = [i for i, x in enumerate(c.lam) if not 320.0 <= x <= 720.0]
        assert (len(bad) >= 1 or len(c.lam) == 1) and np.all(b.E[bad] == 0)
        good = [i for i in range(planes) if i not in bad]
        assert np.all(np.abs(b.E[good]).max(1) > 0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_zero_weight_frame_adds_exactly_nothing(variant):
    """E of the five frames (one of weight 0, one at night) is bit for bit E of the three that count."""
    b = full_batch(variant, False)
    keep = [k for k in range(b.c.K) if b.c.wts[k] != 0 and b.c.ref.suns[k][2] >= 0]
    assert len(keep) == 3
    sub = ss.SunskySequence(b.c.parent, b.c.dirs[keep], [b.c.turb[k] for k in keep], [b.c.wts[k] for k in keep])
    sub.prepare_irradiance(16, 32, wavelengths=b.c.lam)
    np.testing.assert_array_equal(host(sub.irradiance(torch.from_numpy(b.n).cuda())), b.E)


# ---------------------------------------------------------------- 3. launch shapes
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_launch_shapes_are_bitwise_the_full_batch(variant, rotated):
    """Empty batches, 1-7 lanes from unaligned planes, a mask and a row-strided out give, bit for
    bit, the values those lanes have inside the 4,099-lane batch."""
    b = full_batch(variant, rotated)
    seq, P = b.c.seq, b.E.shape[0]
    nrm = torch.from_numpy(b.n).cuda()
    e = host(seq.irradiance(nrm[:, :0]))
    assert e.shape == (P, 0)
    assert ss.lib().sunsky_sequence_irradiance(seq._h, _capi.Vec3In(None, None, None), None, 0, None, 0, None) == 0
    for n in range(1, 8):
        for lo in (0, 1, 4092):
            flat = torch.empty(3 * n + 1, device="cuda")   # planes 4 bytes off any 16-byte boundary
            nn = flat[1:].view(3, n)
            nn.copy_(nrm[:, lo:lo + n])
            assert nn.data_ptr() % 16 == 4
            oflat = torch.full((P * n + 1,), 7.0, device="cuda")
            out = oflat[1:].view(P, n)
            assert seq.irradiance(nn, out=out) is out
            np.testing.assert_array_equal(host(out), b.E[:, lo:lo + n])
            assert float(oflat[0]) == 7.0
    mask = torch.from_numpy((np.arange(N_ALL) % 2).astype(np.uint8)).cuda()
    m = host(seq.irradiance(nrm, active=mask))
    assert np.all(m[:, ::2] == 0) and np.any(b.E[:, ::2] != 0)
    np.testing.assert_array_equal(m[:, 1::2], b.E[:, 1::2])
    wide = torch.full((P, N_ALL + 13), 7.0, device="cuda")   # a row stride larger than n
    out = wide[:, :N_ALL]
    assert out.stride(0) == N_ALL + 13 and seq.irradiance(nrm, out=out) is out
    np.testing.assert_array_equal(host(out), b.E)
    assert np.all(host(wide[:, N_ALL:]) == 7.0)
    assert ss.lib().sunsky_sequence_irradiance(seq._h, _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)]), None, N_ALL,
                                               wide.data_ptr(), N_ALL - 1, None) == 1
    assert b"out_stride" in ss.lib().sunsky_last_error()


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
        assert child.shape == mine.shape and np.any(mine != 0)
        np.testing.assert_array_equal(child, mine)


# ---------------------------------------------------------------- 5. code objects
@pytest.mark.parametrize("variant", VARIANTS)
def test_identity_code_object_gives_the_general_ones_bits(variant, monkeypatch):
    b = full_batch(variant, False)
    monkeypatch.setenv("SUNSKY_AMD_GENERAL_XFORM", "1")
    np.testing.assert_array_equal(host(b.c.seq.irradiance(torch.from_numpy(b.n).cuda())), b.E)


# ---------------------------------------------------------------- 6. graph capture
@pytest.mark.parametrize("variant", VARIANTS)
def test_irradiance_replays_bitwise_from_a_graph(variant):
    """irradiance captured once on a side stream and replayed twice: the output equals the direct
    call bit for bit; nothing is allocated between capture and replay."""
    b = full_batch(variant, False)
    L, P = ss.lib(), b.E.shape[0]
    nrm = torch.from_numpy(b.n).cuda()
    out = torch.zeros((P, N_ALL), device="cuda")

    def call():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.sunsky_sequence_irradiance(b.c.seq._h, _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)]), None, N_ALL,
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
        np.testing.assert_array_equal(out.cpu().numpy(), b.E)
    assert torch.cuda.memory_allocated() == allocated


# ---------------------------------------------------------------- 7. K = 1 end to end
T35 = np.deg2rad(35.0)
K1_NORMALS = {"horizontal": [0.0, 0.0, 1.0], "tilted": [np.sin(T35) * np.cos(0.3), np.sin(T35) * np.sin(0.3), np.cos(T35)]}
K1_DISCRETISATION = 1.95e-4   # measured, see the docstring below


@functools.lru_cache(maxsize=None)
def k1_reference(variant, name):
    """pi x quadrature() of tests/test_direct_diffuse.py for the single emitter of frame 1, and its
    sun part (the same disc cap), computed once."""
    scene = frame_dict(base_dict(), frame_dirs()[1], TURBIDITY[1])
    n = K1_NORMALS[name]
    sun = O.Oracle(dict(scene, sky_scale=0.0), variant, "jit", "f64")
    inf = sun.info()
    return (np.pi * quadrature(scene, variant, n, WL),
            np.pi * _cap_integral(sun, inf["sun_dir_world"], inf["cos_cutoff"], n, WL, 64, 256))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(K1_NORMALS))
def test_one_frame_against_the_oracles_quadrature(variant, name):
    """One frame (20 degrees, T = 2.5, w = 1), 64 x 256 cells, a horizontal and a 35-degree tilted
    receiver, against pi x quadrature(): the fp64 oracle over the sky hemisphere (768 x 1536)
    plus the disc cap.  The bar is 2 x the discretisation of the sky part at 64 x 256 measured
    for this very case with host-only tables on the CPU -- 1.95e-4 relative at the worst (RGB
    1.0e-4 horizontal, 1.9e-4 tilted; spectral 1.1e-4 and 1.95e-4) -- plus 1.5e-3 of the sun
    part (measured 3.3e-4 at the worst).  A wrong omega, ring weight or area_ratio is far outside."""
    lam = tuple(float(x) for x in WL)
    c = sequence(variant, False, "one", (64, 256), lam)
    ref, ref_sun = k1_reference(variant, name)
    n = torch.tensor(K1_NORMALS[name], dtype=torch.float32).reshape(3, 1).cuda()
    E = host(c.seq.irradiance(n))[:, 0].astype(np.float64)
    bound = 2 * K1_DISCRETISATION * (ref - ref_sun) + 1.5e-3 * np.abs(ref_sun)
    print(f"{variant} {name}: E {E}, oracle {ref}, sun part {ref_sun}, worst {np.max(np.abs(E - ref) / bound):.3f} x bound")
    assert np.all(ref - ref_sun > 0) and np.all(np.abs(E - ref) <= bound), np.abs(E - ref) / bound
