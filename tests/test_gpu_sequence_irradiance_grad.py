"""Gradients of a sequence's irradiance on the GPU (sunsky_sequence_prepare_irradiance_grad /
_irradiance_vjp): both gradients per lane and per frame against the fp64 restatement over the
read-back tables (tests/sequence_irradiance_grad_reference.py), against the forward, the
structure of the call, every launch shape and the autograd bridge."""
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
import gpu_sequence_irradiance_grad_worker as W
from sunsky_amd import _capi
from sequence_irradiance_grad_reference import EPS, IrradianceGradReference, frame_sky_tables
from test_gpu_sequence_irradiance import LAMBDAS_32, N_ALL, host, local_of, normals, sequence

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
N_UNIFORM = N_ALL - 20   # the uniform normals come first, then +-z, +-x and the 16 perpendicular to a sun


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cotangents(planes, n):
    """The two cotangents of the tests: standard normal (seed 11) and all ones."""
    return {"normal": np.random.default_rng(11).normal(size=(planes, n)).astype(np.float32),
            "ones": np.ones((planes, n), np.float32)}


@functools.lru_cache(maxsize=None)
def case(variant, rotated, frames="five", size=(16, 32), lam=None):
    """The forward test's sequence with the gradients prepared, the fp64 restatement, and both
    gradients over the 4,099 normals for both cotangents, computed once and shared (read only)."""
    c = sequence(variant, rotated, frames, size, lam)
    c.seq.prepare_irradiance_grad()
    gref = IrradianceGradReference(c.seq, frame_sky_tables(c.parent, c.dirs, c.turb, size, c.lam), c.tw)
    n = normals(c)
    P = gref.r.planes
    d = cotangents(P, N_ALL)
    nrm = cuda(n)
    got = {}
    for name, dd in d.items():
        g = c.seq.irradiance_vjp(nrm, cuda(dd))
        got[name] = (host(g["normals"]), host(g["weights"]))
    return types.SimpleNamespace(c=c, seq=c.seq, gref=gref, n=n, nl=local_of(n, c.tw), d=d, got=got, P=P, K=c.K)


SMALL = [(3, 20), (8, 16), (16, 32)]   # (3, 20): no multiple of the unroll step, fewer entries than a tile
CASES = ([(v, r, "five", s, None) for v in VARIANTS for r in (False, True) for s in SMALL] +
         [("rgb", False, "five", (64, 256), None)] +
         [(v, r, f, (16, 32), None) for v, r in (("rgb", True), ("spectral", False)) for f in ("day", "one")] +
         [("spectral", True, "five", (3, 20), (550.0,)), ("spectral", False, "five", (3, 20), tuple(LAMBDAS_32)),
          ("spectral", True, "five", (16, 32), tuple(LAMBDAS_32))])


# ---------------------------------------------------------------- 1. against the definition
@pytest.mark.parametrize("variant,rotated,frames,size,lam", CASES)
def test_normal_gradient_of_every_lane_against_the_definition(variant, rotated, frames, size, lam):
    """grad_normal of each of the 4,099 lanes and each world axis against the fp64 sum:
    |g - g64| <= 1e-5 M + (n_phi + n_z + K + P + 4) 2^-24 M + slack, M = sum |terms| (the depth
    is the header's), slack the terms whose step can fall either way (|n_l . d| < 8 2^-24 |n_l|
    in fp64).  At least 99 % of the uniform normals have no such term."""
    b = case(variant, rotated, frames, size, lam)
    ref, M, slack = b.gref.normal_grad(b.nl, b.d["normal"])
    clean = np.mean(slack[:, :N_UNIFORM].max(0) == 0)
    assert clean >= 0.99, clean
    got = b.got["normal"][0]
    assert got.shape == (3, N_ALL) and np.all(np.isfinite(got))
    err, bound = np.abs(got.astype(np.float64) - ref), b.gref.normal_bound(M, slack)
    ratio = err / np.maximum(bound, 1e-300)
    print(f"{variant} rotated={rotated} {frames} {size} P={b.P}: worst {ratio.max():.3f} x bound "
          f"({ratio[slack == 0].max():.3f} where there is no slack), "
          f"{100 * clean:.2f} % of the uniform normals without slack")
    assert np.all(err <= bound), (float(ratio.max()), int((err > bound).sum()))
    assert np.abs(got).max() > 0
    if not rotated:
        down = N_ALL - 20 + 1   # the normal (0, 0, -1): no record in front of it
        assert np.all(b.n[:, down] == [0, 0, -1]) and np.all(got[:, down] == 0)


@pytest.mark.parametrize("variant,rotated,frames,size,lam", CASES)
def test_weight_gradient_of_every_frame_against_the_definition(variant, rotated, frames, size, lam):
    """grad_weight[k] of every frame, for the normal and the all-ones cotangent, against the fp64
    restatement: |g - g64| <= (m + 2) 2^-24 M_k + 1e-5 M_k with m the header's depth of the
    reduction at this n.  Night frames get exactly 0; a zero-weight frame gets its E^k."""
    b = case(variant, rotated, frames, size, lam)
    night = b.gref.r.suns[:, 2] < 0
    for name in ("normal", "ones"):
        ref, M = b.gref.weight_grad(b.nl, b.d[name])
        got = b.got[name][1]
        assert got.shape == (b.K,) and np.all(np.isfinite(got))
        err, bound = np.abs(got.astype(np.float64) - ref), b.gref.weight_bound(M, N_ALL)
        ok = ~night
        print(f"{variant} rotated={rotated} {frames} {size} P={b.P} d_out={name}: m = {b.gref.weight_depth(N_ALL)}, "
              f"worst {np.max(err[ok] / bound[ok]):.3f} x bound")
        assert np.all(err <= bound), err / np.maximum(bound, 1e-300)
        assert np.all(got[night] == 0) and np.all(M[ok] > 0)
        if name == "ones":
            assert np.all(got[ok] > 0)
    if frames in ("five", "day"):
        zero = [k for k in range(b.K) if b.c.wts[k] == 0 and not night[k]]
        assert zero and np.all(b.got["ones"][1][zero] > 0)
    if frames == "five":
        assert night[4] and _capi.seq_irr_grad_shape(N_ALL, b.P, size[0] * size[1], b.K)[0] > 1   # several slices


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_zero_weight_frame_gets_the_gradient_it_has_at_weight_one(variant):
    """d E / d w_k does not depend on w: the five frames' weight gradients are bit for bit those of
    the same frames with every weight 1 (the zero-weight frame's included)."""
    b = case(variant, False)
    ones = ss.SunskySequence(b.c.parent, b.c.dirs, b.c.turb, [1.0] * b.K)
    ones.prepare_irradiance(16, 32, wavelengths=b.c.lam)
    ones.prepare_irradiance_grad()
    g = ones.irradiance_vjp(cuda(b.n), cuda(b.d["normal"]), grad={"normals": None, "weights": torch.zeros(b.K, device="cuda")})
    assert b.c.wts[2] == 0 and b.got["normal"][1][2] != 0
    np.testing.assert_array_equal(host(g["weights"]), b.got["normal"][1])


# ---------------------------------------------------------------- 2. against the forward
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_weight_gradient_of_a_one_hot_cotangent_adds_up_to_the_forward(variant, rotated):
    """E is linear in w: for d_out one-hot at (p, r), sum_k w_k grad_weight[k] = E_p(n_r) within the
    forward's accumulation bound plus sum_k w_k times the weight gradient's."""
    b = case(variant, rotated)
    E = host(b.seq.irradiance(cuda(b.n))).astype(np.float64)
    _, _, A = b.gref.r.parts(b.nl)
    fwd = b.gref.r.bound(A)
    w = np.asarray(b.c.wts, np.float64)
    good = [p for p in range(b.P) if np.abs(E[p]).max() > 0]
    for p, r in [(good[0], 0), (good[-1], 1234), (good[len(good) // 2], N_ALL - 1), (good[0], 2049)]:
        d = np.zeros((b.P, N_ALL), np.float32)
        d[p, r] = 1.0
        gw = host(b.seq.irradiance_vjp(cuda(b.n), cuda(d), grad={"normals": None, "weights": torch.zeros(b.K, device="cuda")})
                  ["weights"]).astype(np.float64)
        _, M = b.gref.weight_grad(b.nl, d)
        bound = fwd[p, r] + w @ b.gref.weight_bound(M, N_ALL)
        print(f"{variant} rotated={rotated} (p, r) = ({p}, {r}): E {E[p, r]:.6g}, sum w g {w @ gw:.6g}, "
              f"{abs(w @ gw - E[p, r]) / bound:.3f} x bound")
        assert abs(w @ gw - E[p, r]) <= bound
    assert np.abs(E).max() > 0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_normal_gradient_against_a_central_difference_of_the_forward(variant, rotated):
    """Receivers whose local normal is at least 1e-3 |n_l| away from every step, moved by +-2.5e-4
    along three directions: E is linear between the two fp32 points n+ and n-, so the difference
    has no truncation and  E(n+) - E(n-) = g . (n+ - n-)  up to the forward's rounding bound at both
    points plus the gradient's bound times |n+ - n-|, per plane (d_out one-hot per plane)."""
    b = case(variant, rotated)
    dots = np.abs(b.nl[:N_UNIFORM] @ b.gref.dirs.T) / np.linalg.norm(b.nl[:N_UNIFORM], axis=1, keepdims=True)
    pick = np.flatnonzero(dots.min(1) >= 1e-3)[:64]
    assert pick.size == 64
    n0 = b.n[:, pick]
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(3):
        delta = rng.normal(size=(3, 1))
        delta = (2.5e-4 * delta / np.linalg.norm(delta)).astype(np.float32)
        n_plus, n_minus = (n0 + delta).astype(np.float32), (n0 - delta).astype(np.float32)
        step = n_plus.astype(np.float64) - n_minus.astype(np.float64)           # (3, 64), exact
        E_plus, E_minus = host(b.seq.irradiance(cuda(n_plus))), host(b.seq.irradiance(cuda(n_minus)))
        fd = E_plus.astype(np.float64) - E_minus.astype(np.float64)
        b_plus = b.gref.r.bound(b.gref.r.parts(local_of(n_plus, b.c.tw))[2])
        b_minus = b.gref.r.bound(b.gref.r.parts(local_of(n_minus, b.c.tw))[2])
        for p in range(b.P):
            d = np.zeros((b.P, 64), np.float32)
            d[p] = 1.0
            g = host(b.seq.irradiance_vjp(cuda(n0), cuda(d), grad={"normals": torch.empty((3, 64), device="cuda"),
                                                                     "weights": None})["normals"]).astype(np.float64)
            _, M, slack = b.gref.normal_grad(b.nl[pick], d)
            assert np.all(slack == 0)
            bound = b_plus[p] + b_minus[p] + (np.abs(step) * b.gref.normal_bound(M, slack)).sum(0)
            err = np.abs(fd[p] - (g * step).sum(0))
            if np.abs(fd[p]).max() > 0:
                worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (p, float(np.max(err / np.maximum(bound, 1e-300))))
            # the difference resolves g: somewhere it is larger than the largest allowance (which is mostly
            # the forward's 1e-5 A for table rounding, far above its actual error)
            assert np.abs(fd[p]).max() > bound.max() or np.all(E_plus[p] == 0)
    print(f"{variant} rotated={rotated}: worst {worst:.3f} x bound")


# ---------------------------------------------------------------- 3. structure
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_structure_is_bitwise(variant, rotated):
    """A mask against compaction (normals: any mask; weights: a mask is bit for bit the cotangent
    zeroed at the masked lanes, and a mask over the tail -- which leaves the slices of the rest as
    they are -- is bit for bit the compacted batch), NULL outputs, accumulation into grad_weight,
    overwriting of grad_normal, and two runs."""
    b = case(variant, rotated)
    seq, nrm, d = b.seq, cuda(b.n), cuda(b.d["normal"])
    gn0, gw0 = b.got["normal"]
    # two runs; prefilled outputs: normals overwritten, weights accumulated
    grad = {"normals": torch.full((3, N_ALL), 7.0, device="cuda"), "weights": torch.full((b.K,), 7.0, device="cuda")}
    assert seq.irradiance_vjp(nrm, d, grad=grad) is grad
    np.testing.assert_array_equal(host(grad["normals"]), gn0)
    np.testing.assert_array_equal(host(grad["weights"]), np.float32(7.0) + gw0)
    # NULL outputs
    only_n = seq.irradiance_vjp(nrm, d, grad={"normals": torch.empty((3, N_ALL), device="cuda"), "weights": None})
    only_w = seq.irradiance_vjp(nrm, d, grad={"normals": None, "weights": torch.zeros(b.K, device="cuda")})
    assert only_n["weights"] is None and only_w["normals"] is None
    np.testing.assert_array_equal(host(only_n["normals"]), gn0)
    np.testing.assert_array_equal(host(only_w["weights"]), gw0)
    L = ss.lib()
    v3 = _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)])
    none3 = _capi.Vec3Out(None, None, None)
    assert L.sunsky_sequence_irradiance_vjp(seq._h, v3, None, N_ALL, d.data_ptr(), N_ALL, none3, None, None) == 0   # both NULL
    assert L.sunsky_sequence_irradiance_vjp(seq._h, v3, None, N_ALL, None, N_ALL, none3, None, None) == 1
    assert b"d_out" in L.sunsky_last_error()
    # an interleaved mask
    keep = (np.arange(N_ALL) % 3 != 1)
    m = seq.irradiance_vjp(nrm, d, active=cuda(keep.astype(np.uint8)))
    comp = seq.irradiance_vjp(cuda(b.n[:, keep]), cuda(b.d["normal"][:, keep]))
    gm = host(m["normals"])
    assert np.all(gm[:, ~keep] == 0) and np.any(gn0[:, ~keep] != 0)
    np.testing.assert_array_equal(gm[:, keep], host(comp["normals"]))
    np.testing.assert_array_equal(gm[:, keep], gn0[:, keep])
    zeroed = b.d["normal"].copy()
    zeroed[:, ~keep] = 0
    np.testing.assert_array_equal(host(m["weights"]), host(seq.irradiance_vjp(nrm, cuda(zeroed))["weights"]))
    assert np.any(host(m["weights"]) != gw0)
    # a masked lane may hold anything: NaN normals and cotangents there change nothing
    bad_n, bad_d = b.n.copy(), b.d["normal"].copy()
    bad_n[:, ~keep], bad_d[:, ~keep] = np.nan, np.inf
    mb = seq.irradiance_vjp(cuda(bad_n), cuda(bad_d), active=cuda(keep.astype(np.uint8)))
    np.testing.assert_array_equal(host(mb["normals"]), gm)
    np.testing.assert_array_equal(host(mb["weights"]), host(m["weights"]))
    # a mask over the tail against the compacted batch: the first 4,096 receivers are 4 whole slices
    assert _capi.seq_irr_grad_shape(N_ALL, b.P, 512, b.K) == (5, 1024) and _capi.seq_irr_grad_shape(4096, b.P, 512, b.K) == (4, 1024)
    head = np.arange(N_ALL) < 4096
    mt = seq.irradiance_vjp(nrm, d, active=cuda(head.astype(np.uint8)))
    ct = seq.irradiance_vjp(cuda(b.n[:, :4096]), cuda(b.d["normal"][:, :4096]))
    np.testing.assert_array_equal(host(mt["weights"]), host(ct["weights"]))
    np.testing.assert_array_equal(host(mt["normals"])[:, :4096], host(ct["normals"]))


def test_python_argument_validation():
    """irradiance_vjp refuses, in eval_vjp's style, a cotangent or a grad tensor of the wrong shape,
    type or layout before anything is launched; the outputs given stay untouched."""
    b = case("rgb", False)
    nrm, d = cuda(b.n[:, :8]), cuda(b.d["normal"][:, :8])
    with pytest.raises(ValueError, match="d_out must have shape \\(3, 8\\)"):
        b.seq.irradiance_vjp(nrm, d[:, :7])
    with pytest.raises(ValueError, match="d_out must have shape \\(3, 8\\)"):
        b.seq.irradiance_vjp(nrm, d[:2])
    # a cotangent whose rows are not contiguous is copied, not refused: the contiguous one's bits
    spread = torch.zeros((3, 16), device="cuda")
    spread[:, ::2] = d
    g0, g1 = b.seq.irradiance_vjp(nrm, d), b.seq.irradiance_vjp(nrm, spread[:, ::2])
    for key in ("normals", "weights"):
        np.testing.assert_array_equal(host(g0[key]), host(g1[key]))
    gw = torch.full((b.K,), 7.0, device="cuda")
    for bad in ({"normals": torch.empty((3, 7), device="cuda"), "weights": gw},
                {"normals": torch.empty((3, 8), device="cuda", dtype=torch.float64), "weights": gw},
                {"normals": torch.empty((8, 3), device="cuda").T, "weights": gw},
                {"normals": None, "weights": torch.zeros(b.K + 1, device="cuda")},
                {"normals": None, "weights": torch.zeros(b.K)}):
        with pytest.raises(ValueError, match="must be a contiguous float32 tensor of shape"):
            b.seq.irradiance_vjp(nrm, d, grad=bad)
    assert np.all(host(gw) == 7.0)
    fresh = ss.SunskySequence(b.c.parent, b.c.dirs, b.c.turb, b.c.wts)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        fresh.irradiance_vjp(nrm, d)
    fresh.prepare_irradiance(16, 32)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance_grad first"):
        fresh.irradiance_vjp(nrm, d)


# ---------------------------------------------------------------- 4. launch shapes
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_small_batches_unaligned_planes_and_a_row_stride(variant, rotated):
    """n = 0, and 1 to 7 receivers at three offsets from planes 4 bytes off any 16-byte boundary:
    the normal gradients are bit for bit those lanes of the 4,099-lane batch, the weight gradients
    hold the definition's bound at that n.  A row-strided d_out gives the contiguous one's bits."""
    b = case(variant, rotated)
    seq, P = b.seq, b.P
    gn0, gw0 = b.got["normal"]
    g = seq.irradiance_vjp(torch.empty((3, 0), device="cuda"), torch.empty((P, 0), device="cuda"))
    assert g["normals"].shape == (3, 0) and np.all(host(g["weights"]) == 0)
    assert ss.lib().sunsky_sequence_irradiance_vjp(seq._h, _capi.Vec3In(None, None, None), None, 0, None, 0,
                                                   _capi.Vec3Out(None, None, None), None, None) == 0
    worst = 0.0
    for n in range(1, 8):
        for lo in (0, 1, 4092):
            flat = torch.empty(3 * n + 1, device="cuda")
            nn = flat[1:].view(3, n)
            nn.copy_(cuda(b.n[:, lo:lo + n]))
            dflat = torch.empty(P * n + 1, device="cuda")
            dd = dflat[1:].view(P, n)
            dd.copy_(cuda(b.d["normal"][:, lo:lo + n]))
            oflat = torch.full((3 * n + 1,), 7.0, device="cuda")
            assert nn.data_ptr() % 16 == 4 and dd.data_ptr() % 16 == 4
            g = seq.irradiance_vjp(nn, dd, grad={"normals": oflat[1:].view(3, n), "weights": torch.zeros(b.K, device="cuda")})
            np.testing.assert_array_equal(host(g["normals"]), gn0[:, lo:lo + n])
            assert float(oflat[0]) == 7.0
            ref, M = b.gref.weight_grad(b.nl[lo:lo + n], b.d["normal"][:, lo:lo + n])
            err, bound = np.abs(host(g["weights"]).astype(np.float64) - ref), b.gref.weight_bound(M, n)
            assert np.all(err <= bound), (n, lo, err / np.maximum(bound, 1e-300))
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    print(f"{variant} rotated={rotated}: small batches' weight gradients worst {worst:.3f} x bound")
    wide = torch.full((P, N_ALL + 13), 7.0, device="cuda")
    dd = wide[:, :N_ALL]
    dd.copy_(cuda(b.d["normal"]))
    assert dd.stride(0) == N_ALL + 13
    g = seq.irradiance_vjp(cuda(b.n), dd)
    np.testing.assert_array_equal(host(g["normals"]), gn0)
    np.testing.assert_array_equal(host(g["weights"]), gw0)
    nrm = cuda(b.n)
    gn_c, gw_c = torch.empty((3, N_ALL), device="cuda"), torch.zeros(b.K, device="cuda")   # the stride through the C call itself
    assert ss.lib().sunsky_sequence_irradiance_vjp(seq._h, _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)]), None, N_ALL,
                                                   wide.data_ptr(), N_ALL + 13,
                                                   _capi.Vec3Out(*[gn_c[i].data_ptr() for i in range(3)]), gw_c.data_ptr(),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    np.testing.assert_array_equal(host(gn_c), gn0)
    np.testing.assert_array_equal(host(gw_c), gw0)
    assert ss.lib().sunsky_sequence_irradiance_vjp(seq._h, _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)]), None, N_ALL,
                                                   wide.data_ptr(), N_ALL - 1, _capi.Vec3Out(None, None, None), None,
                                                   None) == 1
    assert b"d_stride" in ss.lib().sunsky_last_error()


def _child(mode, n, tmp_path, env):
    r = subprocess.run([sys.executable, W.__file__, mode, str(n), str(tmp_path)], env=dict(os.environ, **env), timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    return {v: (np.load(tmp_path / f"{v}_normals.npy"), np.load(tmp_path / f"{v}_weights.npy")) for v in W.VARIANTS}


def test_a_grid_smaller_than_the_work_is_bitwise_the_default_grid(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 walks every grid-stride loop several times
    (64 x 256 cells, 64 slices); this process makes the same calls at the default grids."""
    n = W.grid_batch_size()
    child = _child("grid", n, tmp_path, {"SUNSKY_AMD_BLOCKS_PER_CU": "1"})
    for variant in W.VARIANTS:
        gn, gw = W.run(variant, "grid", n)
        assert np.any(gn != 0) and np.all(gw[:4] != 0)
        np.testing.assert_array_equal(child[variant][0], gn)
        np.testing.assert_array_equal(child[variant][1], gw)


def test_a_lowered_workspace_bound_cuts_fewer_slices_and_holds_the_definition(tmp_path):
    """A child process with the workspace bound lowered to 3,200 floats cuts the 4,099 receivers into
    2 slices (RGB) and 1 (spectral) instead of 5: the normal gradients keep their bits, the weight
    gradients hold the definition's bound with the depth of that shape."""
    child = _child("cap", N_ALL, tmp_path, {_capi.SEQ_IRR_GRAD_WORKSPACE_ENV: str(W.CAP_FLOATS)})
    for variant, slices in (("rgb", 2), ("spectral", 1)):
        b = case(variant, False)
        assert _capi.seq_irr_grad_shape(N_ALL, b.P, 512, b.K, W.CAP_FLOATS)[0] == slices
        nl = local_of(W.sphere_normals(N_ALL, 78), None)
        d = W.cotangent(b.P, N_ALL)
        gn, gw = W.run(variant, "cap", N_ALL)   # this process: the default bound, 5 slices
        np.testing.assert_array_equal(child[variant][0], gn)
        ref, M = b.gref.weight_grad(nl, d)
        for got, cap in ((child[variant][1], W.CAP_FLOATS), (gw, _capi.SEQ_IRR_GRAD_WORKSPACE_FLOATS)):
            err, bound = np.abs(got.astype(np.float64) - ref), b.gref.weight_bound(M, N_ALL, cap)
            print(f"{variant} bound {cap}: worst {np.max(err[:4] / bound[:4]):.3f} x bound")
            assert np.all(err <= bound) and got[4] == 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_identity_code_object_gives_the_general_ones_bits(variant, monkeypatch):
    b = case(variant, False)
    monkeypatch.setenv("SUNSKY_AMD_GENERAL_XFORM", "1")
    g = b.seq.irradiance_vjp(cuda(b.n), cuda(b.d["normal"]))
    np.testing.assert_array_equal(host(g["normals"]), b.got["normal"][0])
    np.testing.assert_array_equal(host(g["weights"]), b.got["normal"][1])


@pytest.mark.parametrize("variant", VARIANTS)
def test_irradiance_vjp_replays_bitwise_from_a_graph(variant):
    """irradiance_vjp (all four launches) captured once on a side stream and replayed twice: both
    gradients equal the eager call's bit for bit; nothing is allocated between capture and replay."""
    b = case(variant, False)
    L = ss.lib()
    nrm, d = cuda(b.n), cuda(b.d["normal"])
    gn, gw = torch.zeros((3, N_ALL), device="cuda"), torch.zeros(b.K, device="cuda")

    def call():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.sunsky_sequence_irradiance_vjp(b.seq._h, _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)]), None, N_ALL,
                                                d.data_ptr(), N_ALL, _capi.Vec3Out(*[gn[i].data_ptr() for i in range(3)]),
                                                gw.data_ptr(), st) == 0

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
        gn.zero_()
        gw.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(gn.cpu().numpy(), b.got["normal"][0])
        np.testing.assert_array_equal(gw.cpu().numpy(), b.got["normal"][1])
    assert torch.cuda.memory_allocated() == allocated


# ---------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("variant", VARIANTS)
def test_autograd_bridge_is_bitwise_the_two_calls(variant):
    """sequence_irradiance's value is irradiance's and its gradients are irradiance_vjp's, bit for
    bit, with and without the weights; the weights' gradient arrives on the weights' device."""
    b = case(variant, False)
    seq = ss.SunskySequence(b.c.parent, b.c.dirs, b.c.turb, [1.0] * b.K)
    seq.prepare_irradiance(16, 32, wavelengths=b.c.lam)
    nrm = cuda(b.n).requires_grad_(True)
    w = torch.tensor(b.c.wts, dtype=torch.float32, requires_grad=True)   # on the host
    E = ss.sequence_irradiance(seq, nrm, weights=w)
    np.testing.assert_array_equal(host(E.detach()), host(b.seq.irradiance(cuda(b.n))))
    assert seq.irradiance_grad_prepared
    d = cuda(b.d["normal"])
    E.backward(d)
    np.testing.assert_array_equal(host(nrm.grad), b.got["normal"][0])
    assert w.grad.device.type == "cpu"
    np.testing.assert_array_equal(w.grad.numpy(), b.got["normal"][1])
    nrm2 = cuda(b.n).requires_grad_(True)
    E2 = ss.sequence_irradiance(seq, nrm2)             # the weights as they are now
    np.testing.assert_array_equal(host(E2.detach()), host(E.detach()))
    E2.backward(d)
    np.testing.assert_array_equal(host(nrm2.grad), b.got["normal"][0])
    with pytest.raises(ValueError, match="shape \\(3, n\\)"):
        ss.sequence_irradiance(seq, cuda(b.n).T)


def test_one_gradient_step_on_the_weights_lowers_a_least_squares_loss():
    """Fitting frame weights to a target irradiance on 64 sensors: one step down the gradient from
    all-ones weights lowers the loss."""
    b = case("rgb", False)
    nrm = cuda(b.n[:, :64])
    target = b.seq.irradiance(nrm).clone()
    seq = ss.SunskySequence(b.c.parent, b.c.dirs, b.c.turb, [1.0] * b.K)
    seq.prepare_irradiance(16, 32)
    w = torch.ones(b.K, device="cuda", requires_grad=True)

    def loss_of(weights):
        return ((ss.sequence_irradiance(seq, nrm, weights=weights) - target) ** 2).sum()

    loss = loss_of(w)
    loss.backward()
    g = w.grad
    assert float(loss.detach()) > 0 and float(g.abs().max()) > 0 and float(g[4]) == 0
    # the loss is quadratic in w: the exact minimiser along -g
    with torch.no_grad():
        J = torch.stack([ss.sequence_irradiance(seq, nrm, weights=torch.eye(b.K)[k]).reshape(-1) for k in range(b.K)])
        step = float((g @ g) / (2 * ((g @ J) ** 2).sum()))
        w1 = torch.clamp(w - step * g, min=0.0)
        after = float(loss_of(w1))
    print(f"loss {float(loss.detach()):.6g} -> {after:.6g}")
    assert after < float(loss.detach())


def test_one_gradient_step_on_a_tilt_lowers_a_loss():
    """A panel's tilt theta (normal (sin theta cos phi, sin theta sin phi, cos theta)): one step up the
    gradient of the green irradiance raises it, that is, lowers the loss -E."""
    b = case("rgb", False)
    theta = torch.tensor(0.2, device="cuda", requires_grad=True)
    phi = 1.0

    def loss_of(t):
        n = torch.stack([torch.sin(t) * np.cos(phi), torch.sin(t) * np.sin(phi), torch.cos(t)]).reshape(3, 1).float()
        return -ss.sequence_irradiance(b.seq, n)[1, 0]

    loss = loss_of(theta)
    loss.backward()
    assert float(theta.grad) != 0
    with torch.no_grad():
        after = float(loss_of(theta - 1e-2 * theta.grad / abs(float(theta.grad))))
    print(f"loss {float(loss.detach()):.6g} -> {after:.6g}, d loss / d theta {float(theta.grad):.6g}")
    assert after < float(loss.detach())
