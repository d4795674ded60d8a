"""Gradients of a sequence's irradiance under a horizon profile on the GPU
(sunsky_sequence_irradiance_horizon_vjp, irradiance_vjp(horizon=), sequence_irradiance(horizon=)):
the three gradients per lane, per frame and per (sector, receiver) against the fp64 restatement
(tests/sequence_irradiance_horizon_grad_reference.py), the bit-for-bit identities of the header,
exact finite differences of the forward, the existing kernels, the structure of the call, every
launch shape and the autograd bridge."""
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
import gpu_sequence_irradiance_horizon_grad_worker as W
from sunsky_amd import _capi
from sequence_irradiance_horizon_grad_reference import HorizonGradReference
from test_gpu_sequence_irradiance import LAMBDAS_32, N_ALL, host, local_of, normals, sequence
from test_gpu_sequence_irradiance_horizon import SHAPES

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
N_UNIFORM = N_ALL - 20   # the uniform normals come first, then +-z, +-x and the 16 perpendicular to a sun
KEYS = ("normals", "weights", "horizon")


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


def vjp(seq, n, d, h, **kw):
    """irradiance_vjp(horizon=) of host arrays -> (normals, weights, horizon) as host arrays."""
    g = seq.irradiance_vjp(cuda(n), cuda(d), horizon=cuda(h), **kw)
    return tuple(None if g[k] is None else host(g[k]) for k in KEYS)


@functools.lru_cache(maxsize=None)
def case(variant, rotated, frames="five", size=(16, 32), lam=None, sectors=8):
    """The forward test's sequence with the gradients prepared, the fp64 restatement, and the three
    gradients over the 4,099 normals under 4,099 profiles uniform in [-0.2, 1.2] and under the
    first of them repeated per receiver, for both cotangents: computed once, shared, read only."""
    c = sequence(variant, rotated, frames, size, lam)
    c.seq.prepare_irradiance_grad()
    ref = HorizonGradReference(c.seq, c.tw)
    n = normals(c)
    P = ref.r.planes
    d = cotangents(P, N_ALL)
    h = W.profiles(sectors, N_ALL, 1000 + sectors)
    hs = {"per receiver": h, "shared": np.repeat(h[:, :1], N_ALL, axis=1)}
    got = {(name, kind): vjp(c.seq, n, dd, hh) for name, dd in d.items() for kind, hh in hs.items()}
    return types.SimpleNamespace(c=c, seq=c.seq, ref=ref, n=n, nl=local_of(n, c.tw), d=d, h=h, hs=hs, got=got, P=P, K=c.K,
                                 H=sectors, what=f"{variant} rotated={rotated} {frames} {size} H={sectors} P={P}")


CASES = ([(v, r, "five", s, None, H) for v in VARIANTS for r in (False, True) for s, H in SHAPES] +
         [(v, r, f, (16, 32), None, 8) for v, r in (("rgb", True), ("spectral", False)) for f in ("day", "one")] +
         [("spectral", True, "five", (3, 20), (550.0,), 4), ("spectral", False, "five", (3, 20), tuple(LAMBDAS_32), 4),
          ("spectral", True, "five", (16, 32), tuple(LAMBDAS_32), 8)])


# ---------------------------------------------------------------- 1. every lane against the definition
@pytest.mark.parametrize("variant,rotated,frames,size,lam,sectors", CASES)
def test_normal_gradient_of_every_lane_against_the_definition(variant, rotated, frames, size, lam, sectors):
    """grad_normal of each of the 4,099 lanes and each world axis, under per-receiver profiles and
    under one shared profile, for the normal and the all-ones cotangent, against the fp64 sum within
    HorizonGradReference.normal_bound (derived there).  No lane is left out except through the
    slack term; at least 99 % of the uniform normals have none."""
    b = case(variant, rotated, frames, size, lam, sectors)
    for kind, h in b.hs.items():
        for name in ("normal", "ones"):
            ref, M, slack, partial = b.ref.normal_grad(b.nl, b.d[name], h)
            clean = np.mean(slack[:, :N_UNIFORM].max(0) == 0)
            assert clean >= 0.99, clean
            got = b.got[(name, kind)][0]
            assert got.shape == (3, N_ALL) and np.all(np.isfinite(got))
            err, bound = np.abs(got.astype(np.float64) - ref), b.ref.normal_bound(M, slack, partial)
            ratio = err / np.maximum(bound, 1e-300)
            print(f"{b.what} {kind} d_out={name}: worst {ratio.max():.3f} x bound "
                  f"({ratio[slack == 0].max():.3f} where there is no slack), {100 * clean:.2f} % without slack")
            assert np.all(err <= bound), (float(ratio.max()), int((err > bound).sum()))
            assert np.abs(got).max() > 0
    open_g = host(b.seq.irradiance_vjp(cuda(b.n), cuda(b.d["normal"]), grad={"normals": torch.empty((3, N_ALL), device="cuda"),
                                                                               "weights": None})["normals"])
    assert np.any(open_g != b.got[("normal", "per receiver")][0])   # the horizon is felt


@pytest.mark.parametrize("variant,rotated,frames,size,lam,sectors", CASES)
def test_weight_gradient_of_every_frame_against_the_definition(variant, rotated, frames, size, lam, sectors):
    """grad_weight[k] of every frame against the fp64 restatement within
    HorizonGradReference.weight_bound (the open bound's depth at this n, M_k with v and the
    visibility, fp32(cos v) and v's own rounding).  Night frames get exactly 0."""
    b = case(variant, rotated, frames, size, lam, sectors)
    night = b.ref.r.suns[:, 2] < 0
    for kind, h in b.hs.items():
        for name in ("normal", "ones"):
            ref, M, partial = b.ref.weight_grad(b.nl, b.d[name], h)
            got = b.got[(name, kind)][1]
            assert got.shape == (b.K,) and np.all(np.isfinite(got))
            err, bound = np.abs(got.astype(np.float64) - ref), b.ref.weight_bound(M, partial, N_ALL)
            ok = ~night
            print(f"{b.what} {kind} d_out={name}: worst {np.max(err[ok] / bound[ok]):.3f} x bound")
            assert np.all(err <= bound), err / np.maximum(bound, 1e-300)
            assert np.all(got[night] == 0) and np.all(M[ok] > 0)
            if name == "ones":
                assert np.all(got[ok] > 0)


@pytest.mark.parametrize("variant,rotated,frames,size,lam,sectors", CASES)
def test_horizon_gradient_of_every_entry_against_the_definition(variant, rotated, frames, size, lam, sectors):
    """grad_horizon of every (sector, receiver) against the fp64 restatement within
    HorizonGradReference.horizon_bound.  Not vacuous: at least a quarter of the reference's entries
    are non-zero (1 / 1.4 of the profiles lie in (0, 1), a uniform normal faces a cell with
    probability 1 / 2: about 0.36).  The entries without a partly covered row are exact zeros.  A
    shared profile's gradient is the torch sum of its per-receiver columns."""
    b = case(variant, rotated, frames, size, lam, sectors)
    for kind, h in b.hs.items():
        for name in ("normal", "ones"):
            ref, M, flat = b.ref.horizon_grad(b.nl, b.d[name], h)
            got = b.got[(name, kind)][2]
            assert got.shape == (sectors, N_ALL) and np.all(np.isfinite(got))
            err, bound = np.abs(got.astype(np.float64) - ref), b.ref.horizon_bound(M, flat, sectors)
            live = flat > 0
            print(f"{b.what} {kind} d_out={name}: worst {np.max(err[live] / bound[live]) if live.any() else 0:.3f} x bound, "
                  f"{100 * np.mean(ref != 0):.1f} % of the entries non-zero")
            assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
            assert np.all(got[~live] == 0) and not np.any(np.signbit(got[~live]))
            if kind == "per receiver":
                assert np.mean(ref != 0) >= 0.25, np.mean(ref != 0)
            if name == "ones" and np.all(b.ref.g.terms >= 0):
                assert np.all(got <= 0)   # more horizon, less light
    for shape in ((sectors,), (sectors, 1)):
        g = b.seq.irradiance_vjp(cuda(b.n), cuda(b.d["normal"]), horizon=cuda(b.h[:, 0].reshape(shape)))
        assert tuple(g["horizon"].shape) == shape
        np.testing.assert_array_equal(host(g["horizon"]).reshape(-1),
                                      host(torch.sum(cuda(b.got[("normal", "shared")][2]), dim=1)))
        np.testing.assert_array_equal(host(g["normals"]), b.got[("normal", "shared")][0])
        np.testing.assert_array_equal(host(g["weights"]), b.got[("normal", "shared")][1])


# ---------------------------------------------------------------- 2. bit-for-bit identities
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_open_and_closed_horizons_are_exact(variant, rotated):
    """h = 0, -0, -1 and a shared zero profile: grad_normal and grad_weight are irradiance_vjp's bit
    for bit, grad_horizon exact zeros.  h = 2 and the float above 1: grad_normal and grad_horizon
    exact zeros, grad_weight left as it was."""
    b = case(variant, rotated)
    seq, nrm, d = b.seq, cuda(b.n), cuda(b.d["normal"])
    g0 = seq.irradiance_vjp(nrm, d)
    gn0, gw0 = host(g0["normals"]), host(g0["weights"])
    for sectors in (1, 8, 32):
        opens = [torch.full((sectors, N_ALL), v, device="cuda") for v in (0.0, -0.0, -1.0)]
        opens += [torch.zeros(sectors, device="cuda"), torch.full((sectors, 1), -1.0, device="cuda")]
        for h in opens:
            g = seq.irradiance_vjp(nrm, d, horizon=h)
            np.testing.assert_array_equal(host(g["normals"]), gn0)
            np.testing.assert_array_equal(host(g["weights"]), gw0)
            assert g["horizon"].shape == h.shape and np.all(host(g["horizon"]) == 0)
        above = float(np.nextafter(np.float32(1), np.float32(2)))
        for h in (torch.full((sectors, N_ALL), 2.0, device="cuda"), torch.full((sectors,), 2.0, device="cuda"),
                  torch.full((sectors, N_ALL), above, device="cuda")):
            grad = {"normals": torch.full((3, N_ALL), 7.0, device="cuda"), "weights": cuda(gw0.copy()),
                    "horizon": torch.full(tuple(h.shape), 7.0, device="cuda")}
            seq.irradiance_vjp(nrm, d, grad=grad, horizon=h)
            assert np.all(host(grad["normals"]) == 0) and np.all(host(grad["horizon"]) == 0)
            np.testing.assert_array_equal(host(grad["weights"]).view(np.uint32), gw0.view(np.uint32))
    assert np.any(gn0 != 0) and np.any(gw0 != 0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_masks_and_a_nan_profile(variant, rotated):
    """A masked call: exact zeros at the masked lanes of grad_normal and grad_horizon, the kept
    lanes bit for bit the unmasked call's and the compacted batch's; the weights bit for bit the
    cotangent zeroed at the masked lanes, and under a mask over the tail the compacted batch's.  A
    masked lane may hold anything (NaN normals, cotangents and profiles).  A NaN in an active
    receiver's profile leaves every other receiver's grad_normal and grad_horizon bits intact, its
    lane partner's included."""
    b = case(variant, rotated)
    seq = b.seq
    gn0, gw0, gh0 = b.got[("normal", "per receiver")]
    n, d, h = b.n, b.d["normal"], b.h
    keep = (np.arange(N_ALL) % 3 != 1)
    act = cuda(keep.astype(np.uint8))
    gn, gw, gh = vjp(seq, n, d, h, active=act)
    assert np.all(gn[:, ~keep] == 0) and np.all(gh[:, ~keep] == 0) and np.any(gn0[:, ~keep] != 0) and np.any(gh0[:, ~keep] != 0)
    np.testing.assert_array_equal(gn[:, keep], gn0[:, keep])
    np.testing.assert_array_equal(gh[:, keep], gh0[:, keep])
    cn, _, ch = vjp(seq, n[:, keep], d[:, keep], h[:, keep])
    np.testing.assert_array_equal(gn[:, keep], cn)
    np.testing.assert_array_equal(gh[:, keep], ch)
    zeroed = d.copy()
    zeroed[:, ~keep] = 0
    np.testing.assert_array_equal(gw, vjp(seq, n, zeroed, h)[1])
    assert np.any(gw != gw0)
    bad_n, bad_d, bad_h = n.copy(), d.copy(), h.copy()
    bad_n[:, ~keep], bad_d[:, ~keep], bad_h[:, ~keep] = np.nan, np.inf, np.nan
    for got, want in zip(vjp(seq, bad_n, bad_d, bad_h, active=act), (gn, gw, gh)):
        np.testing.assert_array_equal(got, want)
    # a mask over the tail against the compacted batch: the first 4,096 receivers are 4 whole slices
    assert _capi.seq_irr_grad_shape(N_ALL, b.P, 512, b.K) == (5, 1024) and _capi.seq_irr_grad_shape(4096, b.P, 512, b.K) == (4, 1024)
    head = np.arange(N_ALL) < 4096
    mt = vjp(seq, n, d, h, active=cuda(head.astype(np.uint8)))
    ct = vjp(seq, n[:, :4096], d[:, :4096], h[:, :4096])
    np.testing.assert_array_equal(mt[1], ct[1])
    np.testing.assert_array_equal(mt[0][:, :4096], ct[0])
    np.testing.assert_array_equal(mt[2][:, :4096], ct[2])
    # NaN profiles of active receivers: receiver 5 (the lane partner of 5 + 2050) and the last one
    pairs = (N_ALL + 1) // 2
    nan_h = h.copy()
    for r, sector in ((5, 3), (N_ALL - 1, 0), (pairs + 7, 7)):
        nan_h[sector, r] = np.nan
    gn, _, gh = vjp(seq, n, d, nan_h)
    others = np.ones(N_ALL, bool)
    others[[5, N_ALL - 1, pairs + 7]] = False
    np.testing.assert_array_equal(gn[:, others], gn0[:, others])
    np.testing.assert_array_equal(gh[:, others], gh0[:, others])
    assert others[5 + pairs] and others[7]


# ---------------------------------------------------------------- 3. exact finite differences
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_horizon_gradient_against_a_central_difference_of_the_forward(variant, rotated):
    """E is linear in h inside a row: with h = (i0 + 1/2) / n_z per sector and delta = 1/4 / n_z
    (all exact in fp32), the central difference of irradiance(horizon=) in one sector is the
    derivative up to the forward's rounding: |FD - grad_horizon| <= 2 HorizonReference.bound / (2 delta)
    per entry (d_out one-hot per plane), every entry checked.  The rows are drawn at random, and
    moved on by one where a sun of the sector would lie between the entry's two horizons."""
    b = case(variant, rotated)
    n_z, H = 16, 8
    rng = np.random.default_rng(17)
    i0 = rng.integers(0, n_z, size=(H, N_ALL))
    delta = np.float32(0.25 / n_z)
    # the sun is a step and has no part in the gradient: no sun of a sector may lie between an entry's two
    # horizons (its difference would hold that sun's whole term), so a row that holds one is moved on by one
    length = 32 // H
    for sector in range(H):
        for z in b.ref.hz.sun_z32[b.ref.hz.cols // length == sector]:
            lo, hi = (i0[sector] + 0.25) / n_z, (i0[sector] + 0.75) / n_z
            i0[sector] = np.where((lo <= z) & (z <= hi), (i0[sector] + 1) % n_z, i0[sector])
    h = ((i0 + 0.5) / n_z).astype(np.float32)
    nrm = cuda(b.n)
    gh = []
    for p in range(b.P):
        d = np.zeros((b.P, N_ALL), np.float32)
        d[p] = 1.0
        g = b.seq.irradiance_vjp(nrm, cuda(d), grad={"normals": None, "weights": None,
                                                     "horizon": torch.empty((H, N_ALL), device="cuda")}, horizon=cuda(h))
        gh.append(host(g["horizon"]).astype(np.float64))
    worst, resolved = 0.0, 0
    for sector in range(H):
        hp, hm = h.copy(), h.copy()
        hp[sector] += delta
        hm[sector] -= delta
        assert np.all(hp[sector].astype(np.float64) - hm[sector] == 2 * float(delta))
        Ep, Em = (host(b.seq.irradiance(nrm, horizon=cuda(x))).astype(np.float64) for x in (hp, hm))
        fd = (Ep - Em) / (2 * float(delta))
        bound = np.zeros(fd.shape)
        for x in (hp, hm):
            _, _, A, partial = b.ref.hz.parts(b.nl, x)
            bound += b.ref.hz.bound(A, partial)
        bound /= 2 * float(delta)
        z = b.ref.hz.sun_z32[b.ref.hz.cols // length == sector]
        assert not np.any((z[:, None] >= hp[sector][None, :]) != (z[:, None] >= hm[sector][None, :]))
        for p in range(b.P):
            err = np.abs(fd[p] - gh[p][sector])
            worst = max(worst, float(np.max(err / np.maximum(bound[p], 1e-300))))
            assert np.all(err <= bound[p]), (sector, p, float(np.max(err / np.maximum(bound[p], 1e-300))))
            resolved += int(np.sum(np.abs(fd[p]) > bound[p]))
    print(f"{variant} rotated={rotated}: worst {worst:.3f} x bound, {resolved} entries above their allowance")
    assert resolved > 0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_normal_gradient_against_a_central_difference_of_the_forward(variant, rotated):
    """Receivers whose local normal is at least 1e-3 |n_l| away from every step, moved by +-2.5e-4
    along three directions under their own profiles: E is linear between the two fp32 points, so
    E(n+) - E(n-) = g . (n+ - n-) up to the forward's bound at both points plus the gradient's
    bound times |n+ - n-|, per plane (d_out one-hot per plane)."""
    b = case(variant, rotated)
    dots = np.abs(b.nl[:N_UNIFORM] @ b.ref.g.dirs.T) / np.linalg.norm(b.nl[:N_UNIFORM], axis=1, keepdims=True)
    pick = np.flatnonzero(dots.min(1) >= 1e-3)[:64]
    assert pick.size == 64
    n0, h = b.n[:, pick], b.h[:, pick]
    hd = cuda(h)
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(3):
        delta = rng.normal(size=(3, 1))
        delta = (2.5e-4 * delta / np.linalg.norm(delta)).astype(np.float32)
        n_plus, n_minus = (n0 + delta).astype(np.float32), (n0 - delta).astype(np.float32)
        step = n_plus.astype(np.float64) - n_minus.astype(np.float64)
        E_plus, E_minus = (host(b.seq.irradiance(cuda(x), horizon=hd)) for x in (n_plus, n_minus))
        fd = E_plus.astype(np.float64) - E_minus.astype(np.float64)
        fwd = np.zeros(fd.shape)
        for x in (n_plus, n_minus):
            _, _, A, partial = b.ref.hz.parts(local_of(x, b.c.tw), h)
            fwd += b.ref.hz.bound(A, partial)
        for p in range(b.P):
            d = np.zeros((b.P, 64), np.float32)
            d[p] = 1.0
            g = vjp(b.seq, n0, d, h)[0].astype(np.float64)
            _, M, slack, partial = b.ref.normal_grad(b.nl[pick], d, h)
            assert np.all(slack == 0)
            bound = fwd[p] + (np.abs(step) * b.ref.normal_bound(M, slack, partial)).sum(0)
            err = np.abs(fd[p] - (g * step).sum(0))
            if np.abs(fd[p]).max() > 0:
                worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (p, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.abs(fd[p]).max() > bound.max() or np.all(E_plus[p] == 0)
    print(f"{variant} rotated={rotated}: worst {worst:.3f} x bound")


# ---------------------------------------------------------------- 4. against existing kernels
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_weight_gradient_against_the_series_and_the_forward(variant, rotated):
    """grad_weight[k] for a one-hot cotangent at (p, r) is frame k's irradiance_series(horizon=)
    value there, within the weight bound; sum_k w_k grad_weight[k] is
    irradiance(horizon=) within the forward's bound plus sum_k w_k times the weight bound."""
    b = case(variant, rotated)
    c = b.c
    seq = ss.SunskySequence(c.parent, c.dirs, c.turb, c.wts)   # a sequence of its own: the series is sticky
    seq.prepare_irradiance(16, 32, wavelengths=c.lam)
    seq.prepare_irradiance_grad()
    seq.prepare_irradiance_series()
    nrm, hd = cuda(b.n), cuda(b.h)
    series = host(seq.irradiance_series(nrm, horizon=hd)).astype(np.float64)    # (K, P, n)
    E = host(seq.irradiance(nrm, horizon=hd)).astype(np.float64)
    _, _, A, partial = b.ref.hz.parts(b.nl, b.h)
    fwd = b.ref.hz.bound(A, partial)
    w = np.asarray(c.wts, np.float64)
    good = [p for p in range(b.P) if np.abs(E[p]).max() > 0]
    for p, r in [(good[0], 0), (good[-1], 1234), (good[len(good) // 2], N_ALL - 1), (good[0], 2049)]:
        d = np.zeros((b.P, N_ALL), np.float32)
        d[p, r] = 1.0
        g = seq.irradiance_vjp(nrm, cuda(d), grad={"normals": None, "weights": torch.zeros(b.K, device="cuda")}, horizon=hd)
        gw = host(g["weights"]).astype(np.float64)
        assert g.get("horizon") is None
        _, M, part = b.ref.weight_grad(b.nl, d, b.h)
        wb = b.ref.weight_bound(M, part, N_ALL)
        err = np.abs(gw - series[:, p, r])
        print(f"{variant} rotated={rotated} (p, r) = ({p}, {r}): series worst {np.max(err / np.maximum(wb, 1e-300)):.3f} x bound, "
              f"sum w g {w @ gw:.6g} against E {E[p, r]:.6g}: {abs(w @ gw - E[p, r]) / (fwd[p, r] + w @ wb):.3f} x bound")
        assert np.all(err <= wb), err / np.maximum(wb, 1e-300)
        assert abs(w @ gw - E[p, r]) <= fwd[p, r] + w @ wb
    assert np.abs(E).max() > 0 and np.abs(series).max() > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_zero_weight_frame_gets_the_gradient_it_has_at_weight_one(variant):
    """d E / d w_k does not depend on w: the weight gradients are bit for bit those of the same
    frames with every weight 1 (the zero-weight frame's included); the night frame gets exactly 0."""
    b = case(variant, False)
    ones = ss.SunskySequence(b.c.parent, b.c.dirs, b.c.turb, [1.0] * b.K)
    ones.prepare_irradiance(16, 32, wavelengths=b.c.lam)
    ones.prepare_irradiance_grad()
    g = ones.irradiance_vjp(cuda(b.n), cuda(b.d["normal"]), grad={"normals": None, "weights": torch.zeros(b.K, device="cuda")},
                            horizon=cuda(b.h))
    want = b.got[("normal", "per receiver")][1]
    assert b.c.wts[2] == 0 and want[2] != 0 and want[4] == 0
    np.testing.assert_array_equal(host(g["weights"]), want)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_horizons_on_row_boundaries_and_on_a_suns_height(variant, rotated):
    """h exactly on the row boundaries (v is 0 or 1 everywhere: grad_horizon exact zeros) and, in the
    sectors of the two high suns, exactly the sun's z for some receivers (visible) and the next
    float above it for the others (hidden): the reference's exact fp32 comparison holds in H_p[k]
    (grad_weight) and in the sun part of grad_normal."""
    b = case(variant, rotated)
    r = np.arange(N_ALL)
    h = np.stack([((r + 3 * s) % 17) / 16.0 for s in range(8)]).astype(np.float32)
    gn, gw, gh = vjp(b.seq, b.n, b.d["normal"], h)
    assert np.all(gh == 0)
    cols = b.seq.irradiance_sun_columns()
    assert list(cols // 4) == [0, 2, 4, 6, 0]
    z = np.array([b.seq.frame(k)["sun_dir_local"][2] for k in range(5)], np.float32)
    for k, sector, period in ((1, 2, 3), (3, 6, 2)):
        h[sector] = np.where(r % period == 0, z[k], np.nextafter(z[k], np.float32(2.0)))
    gn, gw, gh = vjp(b.seq, b.n, b.d["normal"], h)
    ref, M, slack, partial = b.ref.normal_grad(b.nl, b.d["normal"], h)
    assert np.all(np.abs(gn - ref) <= b.ref.normal_bound(M, slack, partial))
    ref, M, partial = b.ref.weight_grad(b.nl, b.d["normal"], h)
    assert np.all(np.abs(gw - ref) <= b.ref.weight_bound(M, partial, N_ALL))
    # explicitly: one receiver facing local up, all sectors at frame 1's z / the next float above it
    up = np.asarray(b.c.tw, np.float64)[:3, 2] if rotated else np.array([0.0, 0.0, 1.0])
    one = up[:, None].astype(np.float32)
    lit = [p for p in range(b.P) if b.ref.r.F[p, 1] > 0]
    p = lit[len(lit) // 2]
    d = np.zeros((b.P, 1), np.float32)
    d[p] = 1.0
    seen = vjp(b.seq, one, d, np.full(8, z[1], np.float32))
    hidden = vjp(b.seq, one, d, np.full(8, np.nextafter(z[1], np.float32(2.0)), np.float32))
    dw = float(seen[1][1]) - float(hidden[1][1])
    want = b.ref.r.F[p, 1] * float(z[1])                  # H_p[1] F_1[p] = max(0, n_l . s_1) F_1[p]
    assert abs(dw - want) <= 1e-3 * want, (dw, want)
    dn = local_of(seen[0].astype(np.float64) - hidden[0], b.c.tw)[0]
    want_n = b.ref.r.sun_terms[p, 1] * b.ref.r.suns[1]    # b_r[1] s_1
    assert np.all(np.abs(dn - want_n) <= 1e-3 * np.abs(want_n).max()), (dn, want_n)


# ---------------------------------------------------------------- 5. structure
def c_call(seq, nrm, h, d, n, gn=None, gw=None, gh=None, *, profiles=None, hstride=None, dstride=None, ghstride=None,
           active=None, sectors=None):
    """sunsky_sequence_irradiance_horizon_vjp itself, on torch tensors."""
    return ss.lib().sunsky_sequence_irradiance_horizon_vjp(
        seq._h, _capi.Vec3In(*[nrm[i].data_ptr() for i in range(3)]), h.data_ptr(), h.shape[0] if sectors is None else sectors,
        n if profiles is None else profiles, n if hstride is None else hstride, None if active is None else active.data_ptr(), n,
        d.data_ptr(), n if dstride is None else dstride,
        _capi.Vec3Out(None, None, None) if gn is None else _capi.Vec3Out(*[gn[i].data_ptr() for i in range(3)]),
        None if gw is None else gw.data_ptr(), None if gh is None else gh.data_ptr(), n if ghstride is None else ghstride,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_outputs_accumulation_and_two_runs_are_bitwise(variant, rotated):
    """Two runs; prefilled outputs (normals and horizon overwritten, weights accumulated); NULL
    outputs in every combination, through Python and through the C call."""
    b = case(variant, rotated)
    seq, nrm, d, hd = b.seq, cuda(b.n), cuda(b.d["normal"]), cuda(b.h)
    gn0, gw0, gh0 = b.got[("normal", "per receiver")]
    full = lambda: {"normals": torch.full((3, N_ALL), 7.0, device="cuda"), "weights": torch.full((b.K,), 7.0, device="cuda"),  # noqa: E731
                    "horizon": torch.full((8, N_ALL), 7.0, device="cuda")}
    grad = full()
    assert seq.irradiance_vjp(nrm, d, grad=grad, horizon=hd) is grad
    np.testing.assert_array_equal(host(grad["normals"]), gn0)
    np.testing.assert_array_equal(host(grad["weights"]), np.float32(7.0) + gw0)
    np.testing.assert_array_equal(host(grad["horizon"]), gh0)
    want = {"normals": gn0, "weights": np.float32(7.0) + gw0, "horizon": gh0}
    for mask in range(8):
        grad = full()
        for i, key in enumerate(KEYS):
            if not mask >> i & 1:
                grad[key] = None
        out = seq.irradiance_vjp(nrm, d, grad=grad, horizon=hd)
        for i, key in enumerate(KEYS):
            if mask >> i & 1:
                np.testing.assert_array_equal(host(out[key]), want[key])
            else:
                assert out[key] is None
        t = full()
        assert c_call(seq, nrm, hd, d, N_ALL, *[t[key] if mask >> i & 1 else None for i, key in enumerate(KEYS)]) == 0
        for i, key in enumerate(KEYS):
            np.testing.assert_array_equal(host(t[key]), want[key] if mask >> i & 1 else np.full(t[key].shape, 7.0, np.float32))
    # a grad without a "horizon" entry computes none
    out = seq.irradiance_vjp(nrm, d, grad={"normals": torch.empty((3, N_ALL), device="cuda"), "weights": None}, horizon=hd)
    assert out["horizon"] is None
    np.testing.assert_array_equal(host(out["normals"]), gn0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_small_batches_unaligned_planes_and_row_strides(variant, rotated):
    """n = 0, and 1 to 7 receivers at three offsets from planes 4 bytes off any 16-byte boundary:
    grad_normal and grad_horizon are bit for bit those lanes of the 4,099-lane batch, the weight
    gradients hold the definition's bound at that n.  Row-strided d_out, horizon and grad_horizon
    give the contiguous call's bits and leave the guards between the rows untouched."""
    b = case(variant, rotated)
    seq, P, H = b.seq, b.P, 8
    gn0, gw0, gh0 = b.got[("normal", "per receiver")]
    g = seq.irradiance_vjp(torch.empty((3, 0), device="cuda"), torch.empty((P, 0), device="cuda"),
                           horizon=torch.empty((H, 0), device="cuda"))
    assert g["normals"].shape == (3, 0) and g["horizon"].shape == (H, 0) and np.all(host(g["weights"]) == 0)
    assert ss.lib().sunsky_sequence_irradiance_horizon_vjp(seq._h, _capi.Vec3In(None, None, None), None, 0, 0, 0, None, 0, None, 0,
                                                           _capi.Vec3Out(None, None, None), None, None, 0, None) == 0
    worst = 0.0
    for n in range(1, 8):
        for lo in (0, 1, 4092):
            def off(a):
                flat = torch.full((a.size + 1,), 7.0, device="cuda")
                view = flat[1:].view(a.shape)
                view.copy_(cuda(a))
                assert view.data_ptr() % 16 == 4
                return flat, view
            _, nn = off(b.n[:, lo:lo + n])
            _, dd = off(b.d["normal"][:, lo:lo + n])
            _, hh = off(b.h[:, lo:lo + n])
            oflat, on = off(np.full((3, n), 7.0, np.float32))
            hflat, oh = off(np.full((H, n), 7.0, np.float32))
            g = seq.irradiance_vjp(nn, dd, grad={"normals": on, "weights": torch.zeros(b.K, device="cuda"), "horizon": oh},
                                   horizon=hh)
            np.testing.assert_array_equal(host(g["normals"]), gn0[:, lo:lo + n])
            np.testing.assert_array_equal(host(g["horizon"]), gh0[:, lo:lo + n])
            assert float(oflat[0]) == 7.0 and float(hflat[0]) == 7.0
            ref, M, partial = b.ref.weight_grad(b.nl[lo:lo + n], b.d["normal"][:, lo:lo + n], b.h[:, lo:lo + n])
            err, bound = np.abs(host(g["weights"]).astype(np.float64) - ref), b.ref.weight_bound(M, partial, n)
            assert np.all(err <= bound), (n, lo, err / np.maximum(bound, 1e-300))
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    print(f"{variant} rotated={rotated}: small batches' weight gradients worst {worst:.3f} x bound")
    pad = 13
    wide_d, wide_h = torch.full((P, N_ALL + pad), 7.0, device="cuda"), torch.full((H, N_ALL + pad), 7.0, device="cuda")
    wide_g = torch.full((H, N_ALL + pad), 7.0, device="cuda")
    wide_d[:, :N_ALL].copy_(cuda(b.d["normal"]))
    wide_h[:, :N_ALL].copy_(cuda(b.h))
    g = seq.irradiance_vjp(cuda(b.n), wide_d[:, :N_ALL], grad={"normals": torch.empty((3, N_ALL), device="cuda"),
                                                                 "weights": torch.zeros(b.K, device="cuda"),
                                                                 "horizon": wide_g[:, :N_ALL]}, horizon=wide_h[:, :N_ALL])
    np.testing.assert_array_equal(host(g["normals"]), gn0)
    np.testing.assert_array_equal(host(g["weights"]), gw0)
    np.testing.assert_array_equal(host(wide_g)[:, :N_ALL], gh0)
    assert np.all(host(wide_g)[:, N_ALL:] == 7.0)
    # the strides through the C call itself, and its refusals of short ones
    nrm = cuda(b.n)
    gn_c, gw_c = torch.empty((3, N_ALL), device="cuda"), torch.zeros(b.K, device="cuda")
    wide_g.fill_(7.0)
    kw = dict(hstride=N_ALL + pad, dstride=N_ALL + pad, ghstride=N_ALL + pad)
    assert c_call(seq, nrm, wide_h, wide_d, N_ALL, gn_c, gw_c, wide_g, **kw) == 0
    np.testing.assert_array_equal(host(gn_c), gn0)
    np.testing.assert_array_equal(host(gw_c), gw0)
    np.testing.assert_array_equal(host(wide_g)[:, :N_ALL], gh0)
    assert np.all(host(wide_g)[:, N_ALL:] == 7.0)
    for short, word in (("hstride", b"horizon_stride"), ("dstride", b"d_stride"), ("ghstride", b"grad_horizon_stride")):
        assert c_call(seq, nrm, wide_h, wide_d, N_ALL, gn_c, gw_c, wide_g, **dict(kw, **{short: N_ALL - 1})) == 1
        assert word in ss.lib().sunsky_last_error()


def _child(mode, n, tmp_path, env):
    r = subprocess.run([sys.executable, W.__file__, mode, str(n), str(tmp_path)], env=dict(os.environ, **env), timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    return {v: tuple(np.load(tmp_path / f"{v}_{key}.npy") for key in KEYS) for v in W.VARIANTS}


def test_a_grid_smaller_than_the_work_is_bitwise_the_default_grid(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 walks every grid-stride loop several times
    (64 x 256 cells, 32 sectors, 64 slices); this process makes the same calls at the default grids."""
    n = W.grid_batch_size()
    child = _child("grid", n, tmp_path, {"SUNSKY_AMD_BLOCKS_PER_CU": "1"})
    for variant in W.VARIANTS:
        gn, gw, gh = W.run(variant, "grid", n)
        assert np.any(gn != 0) and np.all(gw[:4] != 0) and np.any(gh != 0)
        for got, want in zip(child[variant], (gn, gw, gh)):
            np.testing.assert_array_equal(got, want)


def test_a_lowered_workspace_bound_cuts_fewer_slices_and_holds_the_definition(tmp_path):
    """A child process with the workspace bound lowered to 3,200 floats cuts the 4,099 receivers into
    2 slices (RGB) and 1 (spectral) instead of 5 at 16 x 32: grad_normal and grad_horizon keep their
    bits, the weight gradients hold the definition's bound with the depth of that shape."""
    child = _child("cap", N_ALL, tmp_path, {_capi.SEQ_IRR_GRAD_WORKSPACE_ENV: str(W.CAP_FLOATS)})
    for variant, slices in (("rgb", 2), ("spectral", 1)):
        b = case(variant, False)
        assert _capi.seq_irr_grad_shape(N_ALL, b.P, 512, b.K, W.CAP_FLOATS)[0] == slices
        nl = local_of(W.sphere_normals(N_ALL, 78), None)
        d, h = W.cotangent(b.P, N_ALL), W.profiles(8, N_ALL, 79)
        gn, gw, gh = W.run(variant, "cap", N_ALL)   # this process: the default bound, 5 slices
        np.testing.assert_array_equal(child[variant][0], gn)
        np.testing.assert_array_equal(child[variant][2], gh)
        ref, M, partial = b.ref.weight_grad(nl, d, h)
        for got, cap in ((child[variant][1], W.CAP_FLOATS), (gw, _capi.SEQ_IRR_GRAD_WORKSPACE_FLOATS)):
            err, bound = np.abs(got.astype(np.float64) - ref), b.ref.weight_bound(M, partial, N_ALL, cap)
            print(f"{variant} bound {cap}: worst {np.max(err[:4] / bound[:4]):.3f} x bound")
            assert np.all(err <= bound) and got[4] == 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_identity_code_object_gives_the_general_ones_bits(variant, monkeypatch):
    b = case(variant, False)
    monkeypatch.setenv("SUNSKY_AMD_GENERAL_XFORM", "1")
    for got, want in zip(vjp(b.seq, b.n, b.d["normal"], b.h), b.got[("normal", "per receiver")]):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("variant", VARIANTS)
def test_irradiance_horizon_vjp_replays_bitwise_from_a_graph(variant):
    """The call (all its launches) captured once on a side stream and replayed twice: the three
    gradients equal the eager call's bit for bit; nothing is allocated between capture and replay."""
    b = case(variant, False)
    nrm, d, hd = cuda(b.n), cuda(b.d["normal"]), cuda(b.h)
    gn, gw, gh = torch.zeros((3, N_ALL), device="cuda"), torch.zeros(b.K, device="cuda"), torch.zeros((8, N_ALL), device="cuda")

    def call():
        assert c_call(b.seq, nrm, hd, d, N_ALL, gn, gw, gh) == 0

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
        for t in (gn, gw, gh):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip((gn, gw, gh), b.got[("normal", "per receiver")]):
            np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.cuda.memory_allocated() == allocated


# ---------------------------------------------------------------- 6. autograd
@pytest.mark.parametrize("variant", VARIANTS)
def test_autograd_bridge_is_bitwise_the_two_calls(variant):
    """sequence_irradiance(horizon=)'s value is irradiance(horizon=)'s and its gradients are
    irradiance_vjp(horizon=)'s, bit for bit, for per-receiver profiles and for a shared one (whose
    gradient is the torch sum of the per-receiver planes); without a horizon it is the open call."""
    b = case(variant, False)
    seq = ss.SunskySequence(b.c.parent, b.c.dirs, b.c.turb, [1.0] * b.K)
    seq.prepare_irradiance(16, 32, wavelengths=b.c.lam)
    d = cuda(b.d["normal"])
    for kind, hh in (("per receiver", b.h), ("shared", b.h[:, 0])):
        nrm = cuda(b.n).requires_grad_(True)
        w = torch.tensor(b.c.wts, dtype=torch.float32, requires_grad=True)   # on the host
        hz = cuda(hh).requires_grad_(True)
        E = ss.sequence_irradiance(seq, nrm, weights=w, horizon=hz)
        np.testing.assert_array_equal(host(E.detach()), host(b.seq.irradiance(cuda(b.n), horizon=cuda(hh))))
        E.backward(d)
        gn, gw, gh = b.got[("normal", kind)]
        np.testing.assert_array_equal(host(nrm.grad), gn)
        assert w.grad.device.type == "cpu"
        np.testing.assert_array_equal(w.grad.numpy(), gw)
        assert hz.grad.shape == hz.shape
        np.testing.assert_array_equal(host(hz.grad), gh if kind == "per receiver" else host(torch.sum(cuda(gh), dim=1)))
    # a horizon that does not require grad gets none; the open call is untouched
    nrm = cuda(b.n).requires_grad_(True)
    hz = cuda(b.h)
    ss.sequence_irradiance(seq, nrm, horizon=hz).backward(d)
    assert hz.grad is None
    np.testing.assert_array_equal(host(nrm.grad), b.got[("normal", "per receiver")][0])
    nrm = cuda(b.n).requires_grad_(True)
    E = ss.sequence_irradiance(seq, nrm)
    np.testing.assert_array_equal(host(E.detach()), host(b.seq.irradiance(cuda(b.n))))
    E.backward(d)
    np.testing.assert_array_equal(host(nrm.grad), host(b.seq.irradiance_vjp(cuda(b.n), d)["normals"]))
    with pytest.raises(ValueError, match="horizon must be a float32 tensor"):
        ss.sequence_irradiance(seq, nrm, horizon=b.h)


@pytest.mark.parametrize("variant", VARIANTS)
def test_autograd_with_one_receiver_and_a_shared_profile(variant):
    """One sensor under an (H,) profile that requires grad: the gradient arrives in the shape given and
    is bit for bit that receiver's column of the 4,099-lane batch; irradiance_vjp returns the same."""
    b = case(variant, False)
    r = 1234
    nrm = cuda(b.n[:, r:r + 1]).requires_grad_(True)
    hz = cuda(b.h[:, r]).requires_grad_(True)
    d = cuda(b.d["normal"][:, r:r + 1])
    E = ss.sequence_irradiance(b.seq, nrm, horizon=hz)
    E.backward(d)
    gn, _, gh = b.got[("normal", "per receiver")]
    assert hz.grad.shape == (8,) and np.any(gh[:, r] != 0)
    np.testing.assert_array_equal(host(hz.grad), gh[:, r])
    np.testing.assert_array_equal(host(nrm.grad), gn[:, r:r + 1])
    g = b.seq.irradiance_vjp(nrm.detach(), d, horizon=hz.detach())
    assert g["horizon"].shape == (8,)
    np.testing.assert_array_equal(host(g["horizon"]), gh[:, r])
    g = b.seq.irradiance_vjp(nrm.detach(), d, horizon=hz.detach().reshape(8, 1))
    assert g["horizon"].shape == (8, 1)
    np.testing.assert_array_equal(host(g["horizon"])[:, 0], gh[:, r])


def test_one_gradient_step_on_a_tilt_under_a_horizon_lowers_a_loss():
    """A panel's tilt theta behind a hill to its south-east: one step up the gradient of the green
    irradiance under the horizon raises it, that is, lowers the loss -E."""
    b = case("rgb", False)
    theta = torch.tensor(0.6, device="cuda", requires_grad=True)
    phi = 1.0
    hz = torch.tensor([0.45, 0.3, 0.05, 0.0, 0.0, 0.1, 0.2, 0.45], device="cuda")

    def loss_of(t):
        n = torch.stack([torch.sin(t) * np.cos(phi), torch.sin(t) * np.sin(phi), torch.cos(t)]).reshape(3, 1).float()
        return -ss.sequence_irradiance(b.seq, n, horizon=hz)[1, 0]

    loss = loss_of(theta)
    loss.backward()
    assert float(theta.grad) != 0
    with torch.no_grad():
        after = float(loss_of(theta - 1e-2 * theta.grad / abs(float(theta.grad))))
    print(f"loss {float(loss.detach()):.6g} -> {after:.6g}, d loss / d theta {float(theta.grad):.6g}")
    assert after < float(loss.detach())


def test_one_gradient_step_on_a_horizon_value_lowers_a_loss():
    """Fitting a shared horizon to the irradiance measured on 64 sensors: one step down the gradient
    of the least-squares loss from a horizon that is too high lowers the loss."""
    b = case("rgb", False)
    nrm = cuda(b.n[:, :64])
    true = torch.tensor([(i0 + 0.5) / 16 for i0 in (2, 4, 1, 3, 5, 2, 3, 1)], device="cuda")
    target = b.seq.irradiance(nrm, horizon=true).clone()
    hz = (true + 0.125 / 16).requires_grad_(True)          # inside the same rows: the loss is quadratic in h

    def loss_of(x):
        return ((ss.sequence_irradiance(b.seq, nrm, horizon=x) - target) ** 2).sum()

    loss = loss_of(hz)
    loss.backward()
    g = hz.grad
    assert float(loss.detach()) > 0 and float(g.abs().max()) > 0 and g.shape == hz.shape
    with torch.no_grad():
        # d residual / d step along -g by a difference inside the rows (E is linear there): the exact minimiser
        eps = 0.0625 / 16 / float(g.abs().max())
        r0 = ss.sequence_irradiance(b.seq, nrm, horizon=hz.detach()) - target
        r1 = ss.sequence_irradiance(b.seq, nrm, horizon=hz.detach() - eps * g) - target
        slope = (r1 - r0) / eps
        step = min(float(-(r0 * slope).sum() / (slope * slope).sum()), 0.25 / 16 / float(g.abs().max()))
        after = float(loss_of(hz.detach() - step * g))
    print(f"loss {float(loss.detach()):.6g} -> {after:.6g}")
    assert step > 0 and after < float(loss.detach())
