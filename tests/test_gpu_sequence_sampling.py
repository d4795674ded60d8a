"""Importance sampling of frame sequences on the GPU (sunsky_sequence_sample_direction /
_pdf_direction): the tables, the pdf and the sample map per lane against the numpy restatement
(tests/sequence_sampling_reference.py), the sampler against its own pdf, an end-to-end
irradiance, every launch shape, graph capture and K = 1 against the single emitter."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from scipy.special import gammaincc

import oracle as O
import sunsky_amd as ss
import gpu_sequence_sampling_worker as W
from chi2 import pool_chi2
from sequence_cases import (DAY_TIMES, DAY_TURBIDITY, DAY_WEIGHTS, LAMBDAS, TURBIDITY, WEIGHTS, base_dict, batch_wo,
                            frame_dict, frame_dirs, rotation, to_world_dirs)
from sequence_sampling_reference import NODE_LAMBDAS, SamplingReference, cell_centres, luminance
from test_direct_diffuse import _cap_integral, _gl

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
PRECISIONS = ["fast", "reference"]
TABLES = [(8, 16), (16, 32), (64, 256)]
EPS = 2.0 ** -24
CAP = 0.005   # at most 0.5 % of lanes may be left out of a per-lane comparison


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def soa(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def local_of(d_world, tw):
    """(3, n) world directions -> (n, 3) local, fp64 (R^-1 = R^T)."""
    d = np.asarray(d_world, np.float64).T
    return d if tw is None else d @ np.asarray(tw, np.float64)[:3, :3]


def uniform(n, seed=5):
    return np.random.default_rng(seed).random((2, n), dtype=np.float32)


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6 * max(np.abs(ref).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def sequence(variant, precision, rotated, frames="five", size=(64, 256), **kw):
    """A parent, its sequence with the sampling tables prepared, and the numpy restatement."""
    tw = rotation() if rotated else None
    base = base_dict(**dict(kw, **({"to_world": tw} if rotated else {})))
    parent = ss.SunskyEmitter(base, variant, precision=precision)
    if frames == "five":
        dirs, turb, wts = frame_dirs(tw), TURBIDITY, WEIGHTS
    elif frames == "day":
        m = np.asarray(parent.get_param("to_world"), np.float32)[:3, :3]
        dirs = np.stack([m @ ss.sun_coordinates(*t) for t in DAY_TIMES]).astype(np.float32)
        turb, wts = DAY_TURBIDITY, DAY_WEIGHTS
    else:   # K = 1
        dirs, turb, wts = frame_dirs(tw)[1:2], TURBIDITY[1:2], [1.0]
    seq = ss.SunskySequence(parent, dirs, turb, wts)
    seq.prepare_sampling(*size)
    ref = SamplingReference(seq, parent.info()["cos_cutoff"])
    lam = LAMBDAS if variant == "spectral" else None
    return types.SimpleNamespace(base=base, tw=tw, parent=parent, seq=seq, ref=ref, dirs=dirs, turb=turb, wts=wts,
                                 K=len(turb), lam=lam, variant=variant, precision=precision)


@functools.lru_cache(maxsize=None)
def samples(variant, precision, rotated, frames="five", size=(64, 256), n=1 << 16, **kw):
    """sample_direction over n fixed u, pdf_direction and sequence.eval at the sampled directions,
    computed once and shared (read only)."""
    c = sequence(variant, precision, rotated, frames, size, **kw)
    u = uniform(n)
    ds, w = c.seq.sample_direction(None, torch.from_numpy(u).cuda(), c.lam)
    p = c.seq.pdf_direction(None, ds)
    e = c.seq.eval(-ds.d, c.lam)
    d = host(ds.d)
    return types.SimpleNamespace(c=c, u=u, d=d, local=local_of(d, c.tw), pdf=host(ds.pdf), w=host(w), p=host(p),
                                 e=host(e), dist=host(ds.dist), pos=host(ds.p))


def finite_eval(s):
    """Lanes where sequence.eval(-ds.d) is finite.  eval takes cos theta = d.z as given, and a
    unit fp32 vector next to the zenith can have z = 1 + 6e-8: inside a disc there the elevation
    pi/2 - acos(z) is NaN, in the single emitter's eval as well.  The sampler's weight is 0 on
    such a lane (the quotient is not finite).  The sampler clamps its local sun picks to z <= 1,
    so with an identity to_world there is none; a rotated round trip can still make a few."""
    fin = np.isfinite(s.e).all(axis=0)
    assert np.all(s.w[:, ~fin] == 0) and (~fin).mean() < 1e-3
    assert np.all(s.local[~fin, 2] > 1.0 - 1e-6)
    return fin


# ---------------------------------------------------------------- 1. tables
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size", TABLES)
def test_device_table_matches_the_host_table_and_the_public_eval(variant, size):
    """The device table within 1e-5 of the host-only table's largest entry, and against
    sequence.eval of a sun_scale-0 sequence at the cell centres at the accumulation bar
    1e-5 max f + (K + 2) 2^-24 sum_k w_k |v_k| (the luminances are >= 0: the sum is the value)."""
    c = sequence(variant, "reference", False, "five", size)
    f = c.ref.f.astype(np.float64)
    hp = ss.SunskyEmitter(c.base, variant, device="host")
    hs = ss.SunskySequence(hp, c.dirs, c.turb, c.wts)
    hs.prepare_sampling(*size)
    fh = hs.sampling_table("sky").astype(np.float64)
    print(f"{variant} {size}: device vs host table {np.abs(f - fh).max() / fh.max():.3e} of the largest entry")
    assert np.abs(f - fh).max() <= 1e-5 * fh.max()
    for name in ("B", "q"):
        np.testing.assert_allclose(c.seq.sampling_table(name), hs.sampling_table(name), rtol=1e-5, atol=0)
    assert abs(c.seq.sampling_info()["w_sky"] - hs.sampling_info()["w_sky"]) <= 1e-5
    sky_parent = ss.SunskyEmitter(dict(c.base, sun_scale=0.0), variant, precision="reference")
    sky_seq = ss.SunskySequence(sky_parent, c.dirs, c.turb, c.wts)
    lam = NODE_LAMBDAS if variant == "spectral" else None
    v = host(sky_seq.eval(soa(-cell_centres(*size)), lam))
    y = luminance(v.T, variant == "spectral")
    bound = 1e-5 * f.max() + (c.K + 2) * EPS * np.abs(y)
    err = np.abs(f.reshape(-1) - y)
    print(f"vs sequence.eval: worst {np.max(err / bound):.3f} x bound")
    assert np.all(err <= bound), (np.max(err / bound), int((err > bound).sum()))


@pytest.mark.parametrize("variant", VARIANTS)
def test_suns_match_the_gpus_single_emitters(variant):
    """B_k against Y of the GPU's own single emitter (sky_scale 0) at its disc centre, 1e-5."""
    c = sequence(variant, "reference", False, "five", (8, 16))
    lam = NODE_LAMBDAS if variant == "spectral" else None
    for k in range(c.K):
        s = c.seq.frame(k)["sun_dir_local"]
        em = ss.SunskyEmitter(dict(frame_dict(c.base, c.dirs[k], c.turb[k]), sky_scale=0.0), variant, precision="reference")
        wi = soa(-s[None, :])
        v = host(em.eval(ss.SurfaceInteraction3f(wi=wi)) if lam is None else em.eval_spectral_broadcast(wi, lam))
        y = float(luminance(v.T, variant == "spectral")[0])
        print(f"frame {k}: B {c.ref.B[k]:.6g}, emitter {y:.6g}")
        assert (c.ref.B[k] == 0 and y == 0) if s[2] < 0 else abs(c.ref.B[k] - y) <= 1e-5 * y


# ---------------------------------------------------------------- 2. pdf per lane
PDF_CASES = [(v, p, r, f, s) for v in VARIANTS for p in PRECISIONS for r in (False, True)
             for f, s in (("five", (64, 256)), ("five", (8, 16)), ("day", (16, 32)), ("one", (16, 32)))]


@pytest.mark.parametrize("variant,precision,rotated,frames,size", PDF_CASES)
def test_pdf_direction_per_lane(variant, precision, rotated, frames, size):
    """pdf_direction against the numpy pdf over batch_wo (hemisphere, in-disc and below-horizon
    directions), 1e-5 relative; lanes at a cell boundary or a cone edge left out, <= 0.5 %."""
    c = sequence(variant, precision, rotated, frames, size)
    wo = batch_wo(list(c.ref.suns), c.parent.info()["sun_half_aperture"])
    d_t = soa(to_world_dirs(wo, c.tw))
    got = host(c.seq.pdf_direction(None, d_t))
    ref, leave = c.ref.pdf(local_of(host(d_t), c.tw))
    keep = ~leave
    err = rel_err(got[keep], ref[keep])
    in_cone = c.ref.cone_hits(wo)[0][:, c.ref.q > 0].any(axis=1) & (wo[:, 2] >= 0)
    print(f"max rel {err.max():.3e}, left out {leave.mean():.2e}, in-cone lanes {int(in_cone.sum())}")
    assert in_cone.sum() >= 64
    assert leave.mean() <= CAP
    assert err.max() <= 1e-5
    assert np.all(got[wo[:, 2] < 0] == 0) and (wo[:, 2] < 0).sum() >= 16
    mask = torch.from_numpy((np.arange(wo.shape[0]) % 2).astype(np.uint8)).cuda()
    got_m = host(c.seq.pdf_direction(None, d_t, active=mask))
    assert np.all(got_m[::2] == 0)
    np.testing.assert_array_equal(got_m[1::2], got[1::2])


# ---------------------------------------------------------------- 3. sample per lane
SAMPLE_CASES = [(v, p, r, f, s) for v in VARIANTS for p in PRECISIONS for r in (False, True)
                for f, s in (("five", (64, 256)), ("day", (16, 32)))] + [("rgb", "fast", False, "one", (8, 16))]


@pytest.mark.parametrize("variant,precision,rotated,frames,size", SAMPLE_CASES)
def test_sample_direction_per_lane(variant, precision, rotated, frames, size):
    """d, pdf and weight of 2^16 samples against the numpy map on the same u.  Directions:
    |dd| < 2e-6 at the 99.9th percentile, < 1e-4 at most.  pdf and weight: 1e-5 at the GPU's own
    directions (the weight against sequence.eval there over the numpy pdf).  Left out: u within
    1e-6 of a CDF entry or of w_sky, and for the pdf the numpy pdf's cell-boundary band; <= 0.5 %
    in all.  Cone-edge lanes are NOT left out: a sun pick is uniform over its cone, so
    3e-7 / (1 - cos_cutoff) = 2.7 % of the sun picks lie within 3e-7 of the edge at the default
    aperture, several times the cap; such a lane is held to one of its two admissible values
    (SamplingReference.pdf, resolve)."""
    s = samples(variant, precision, rotated, frames, size)
    r = s.c.ref
    m = r.sample(s.u)
    pref, pleave = r.pdf(s.local, resolve=s.pdf)
    leave = m["leave_out"] | pleave
    keep = ~leave
    dd = np.linalg.norm(s.local - m["d"], axis=1)[~m["leave_out"]]
    print(f"left out {leave.mean():.2e}; |dd| 99.9 % {np.quantile(dd, 0.999):.3e}, max {dd.max():.3e}; "
          f"sky picks {m['pick_sky'].mean():.4f} (w_sky {float(r.w_sky):.4f})")
    assert leave.mean() <= CAP
    assert np.quantile(dd, 0.999) < 2e-6 and dd.max() < 1e-4
    active = s.local[:, 2] >= 0
    # the kernel's own activity: pdf 0 and weight 0 exactly where the sample is below the horizon
    band = np.abs(s.local[:, 2]) < 1e-6
    assert np.all((s.pdf > 0)[~band] == active[~band])
    assert np.all(s.w[:, s.pdf == 0] == 0)
    perr = rel_err(s.pdf[keep], pref[keep])
    keep_w = keep & finite_eval(s)
    wref = np.where(pref > 0, s.e.astype(np.float64) / np.where(pref > 0, pref, 1.0), 0.0)
    werr = rel_err(s.w[:, keep_w], wref[:, keep_w])
    print(f"pdf max rel {perr.max():.3e}, weight max rel {werr.max():.3e}")
    assert perr.max() <= 1e-5 and werr.max() <= 1e-5
    # ds.dist / ds.p from the snapshot's bounding sphere with it.p = origin
    inf = s.c.parent.info()
    dist = 2 * max(inf["bsphere_radius"], float(np.linalg.norm(inf["bsphere_center"])))
    assert np.allclose(s.dist, dist, rtol=1e-6) and np.allclose(s.pos, s.d * s.dist, rtol=1e-6, atol=1e-6 * dist)
    if variant == "spectral":
        assert np.all(s.w[LAMBDAS.index(300.0)] == 0) and np.any(s.w[0] != 0)


# ---------------------------------------------------------------- 4. consistency
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_consistency_identity(variant, precision):
    """Identity to_world: ds.pdf is pdf_direction(ds.d) bit for bit, and weight x pdf is
    sequence.eval(-ds.d) within 1e-5 on every active lane."""
    s = samples(variant, precision, False)
    np.testing.assert_array_equal(s.pdf, s.p)
    act = (s.pdf > 0) & finite_eval(s)
    assert act.mean() > 0.9
    err = rel_err(s.w[:, act].astype(np.float64) * s.pdf[act], s.e[:, act])
    print(f"weight x pdf vs eval: max rel {err.max():.3e}")
    assert err.max() <= 1e-5


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_consistency_rotated_wide_cones(variant, precision):
    """Rotated to_world and a 5 degree sun_aperture (cones that overlap the horizon and cover
    many cells): the same two equalities at 1e-5, cone-edge lanes (|dot - cos_cutoff| < 3e-7)
    left out, <= 0.5 %."""
    s = samples(variant, precision, True, sun_aperture=5.0)
    _, edge = s.c.ref.cone_hits(s.local)
    assert edge.mean() <= CAP
    keep = ~edge
    perr = rel_err(s.pdf[keep], s.p[keep])
    act = keep & (s.pdf > 0) & finite_eval(s)
    err = rel_err(s.w[:, act].astype(np.float64) * s.pdf[act], s.e[:, act])
    sun_picks = s.u[0] >= s.c.ref.w_sky
    print(f"pdf vs pdf_direction {perr.max():.3e}, weight x pdf vs eval {err.max():.3e}; edge {edge.mean():.2e}, "
          f"sun picks {sun_picks.mean():.3f}, below the horizon {(s.local[:, 2] < 0).mean():.3f}")
    assert perr.max() <= 1e-5 and err.max() <= 1e-5
    assert sun_picks.sum() > 100 and (s.local[:, 2] < 0).sum() > 0


# ---------------------------------------------------------------- 5. the sampler follows its pdf
def test_the_sampler_follows_its_pdf():
    """2^20 samples on a 16 x 32 table.  Sky picks histogrammed into the table's own cells against
    N_sky f_ij / S, and their in-cell positions pooled over cells into 8 x 8 bins against uniform
    (pool_chi2, p > 0.01).  Sun picks: inside their frame's cone, per-frame counts within 5
    binomial sigma of N_sun q_k, none for the night and the zero-weight frame; the sky fraction
    within 5 sigma of w_sky."""
    n = 1 << 20
    s = samples("rgb", "fast", False, "five", (16, 32), n)
    r = s.c.ref
    m = r.sample(s.u)
    sky = m["pick_sky"]
    n_sky, n_sun, w = int(sky.sum()), int((~sky).sum()), float(r.w_sky)
    assert abs(n_sky - n * w) <= 5 * np.sqrt(n * w * (1 - w))
    d = s.local[sky]
    zr, pc = d[:, 2] * r.n_z, np.mod(np.arctan2(d[:, 1], d[:, 0]), 2 * np.pi) / r.dphi
    row, col = np.clip(np.floor(zr), 0, r.n_z - 1).astype(int), np.clip(np.floor(pc), 0, r.n_phi - 1).astype(int)
    obs = np.bincount(row * r.n_phi + col, minlength=r.n_z * r.n_phi).astype(np.float64)
    exp = n_sky * r.f.astype(np.float64).reshape(-1) / r.S
    chsq, dof, _, _ = pool_chi2(obs, exp)
    p_cells = float(gammaincc(dof / 2.0, chsq / 2.0))
    bz, bp = np.clip(((zr - row) * 8).astype(int), 0, 7), np.clip(((pc - col) * 8).astype(int), 0, 7)
    obs_in = np.bincount(bz * 8 + bp, minlength=64).astype(np.float64)
    chsq_in, dof_in, _, _ = pool_chi2(obs_in, np.full(64, n_sky / 64.0))
    p_in = float(gammaincc(dof_in / 2.0, chsq_in / 2.0))
    print(f"cells: chi2 {chsq:.1f} / {dof} dof, p {p_cells:.3f}; in-cell: chi2 {chsq_in:.1f} / {dof_in} dof, p {p_in:.3f}")
    assert p_cells > 0.01 and p_in > 0.01
    k = m["frame"][~sky]
    dots = np.einsum("ij,ij->i", s.local[~sky], r.suns[k].astype(np.float64))
    sure = ~m["leave_out"][~sky]   # u away from a CDF entry: the numpy map's frame is the kernel's
    assert np.all(dots[sure] >= float(r.cos_cutoff) - 1e-6), (dots[sure] - float(r.cos_cutoff)).min()
    counts = np.bincount(k, minlength=r.K)
    q = r.q.astype(np.float64)
    print("sun picks per frame", counts.tolist(), "expected", np.round(n_sun * q, 1).tolist())
    assert np.all(np.abs(counts - n_sun * q) <= 5 * np.sqrt(n_sun * q * (1 - q)) + 1e-9)
    assert counts[4] == 0 and counts[2] == 0 and q[4] == 0 and q[2] == 0   # night frame, zero weight


# ---------------------------------------------------------------- 6. unbiased end to end
def irradiance(s):
    """mean(weight cos theta) per channel and its standard error (identity to_world)."""
    x = s.w.astype(np.float64) * np.maximum(s.local[:, 2], 0.0)[None, :]
    return x.mean(1), x.std(1) / np.sqrt(x.shape[1])


def test_sky_only_irradiance_is_unbiased():
    """Horizontal irradiance of a sky-only sequence (sun_scale 0) over 2^22 samples against a
    Gauss-Legendre x trapezoid quadrature of sequence.eval: within 5 standard errors + 1e-3."""
    s = samples("rgb", "fast", False, "five", (64, 256), 1 << 22, sun_scale=0.0)
    est, se = irradiance(s)
    mu, wmu = _gl(256, 0.0, 1.0)
    phi = (np.arange(512) + 0.5) * (2 * np.pi / 512)
    M, P = np.meshgrid(mu, phi, indexing="ij")
    st = np.sqrt(1 - M * M)
    wdir = np.stack([st * np.cos(P), st * np.sin(P), M], -1).reshape(-1, 3)
    L = host(s.c.seq.eval(soa(-wdir))).astype(np.float64)
    q = (L * (wdir[:, 2] * np.repeat(wmu, 512) * (2 * np.pi / 512))[None, :]).sum(1)
    print(f"sky: estimate {est}, quadrature {q}, se {se}, dev/se {np.abs(est - q) / se}")
    assert s.c.seq.sampling_info()["w_sky"] == 1.0
    assert np.all(np.abs(est - q) <= 5 * se + 1e-3 * q)


def test_sun_only_irradiance_is_unbiased():
    """The same for a sun-only sequence (sky_scale 0) against the per-disc quadrature of
    tests/test_direct_diffuse.py (fp64 oracle over each cone): within 5 se + 1.5e-3, the
    measured fp32 cone-edge deficit.  Measured: -4.1e-4 to -6.6e-4 relative
    (0.8-1.0 se); -2.7e-3 to -3.0e-3 before the sampler clamped its sun picks to z <= 1 (the
    89.9 degree sun's picks with z = 1 + 6e-8 evaluate to NaN and weigh 0)."""
    s = samples("rgb", "fast", False, "five", (64, 256), 1 << 22, sky_scale=0.0)
    est, se = irradiance(s)
    q = np.zeros(3)
    for k in range(s.c.K):
        if s.c.wts[k] == 0:
            continue
        o = O.Oracle(dict(frame_dict(s.c.base, s.c.dirs[k], s.c.turb[k]), sky_scale=0.0), "rgb", "jit", "f64")
        inf = o.info()
        q += s.c.wts[k] * np.pi * _cap_integral(o, inf["sun_dir_world"], inf["cos_cutoff"], [0.0, 0.0, 1.0], None, 64, 256)
    print(f"sun: estimate {est}, quadrature {q}, se {se}, rel dev {(est - q) / q}")
    assert s.c.seq.sampling_info()["w_sky"] == 0.0
    assert np.all(np.abs(est - q) <= 5 * se + 1.5e-3 * q)


# ---------------------------------------------------------------- 7. launch shapes
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("rotated", [False, True])
def test_launch_shapes_are_bitwise_the_full_batch(variant, precision, rotated):
    """Empty batches, 1-7 lanes, masks and unaligned planes give, bit for bit, the samples those
    lanes have inside the 4,099-lane batch."""
    c = sequence(variant, precision, rotated, "five", (16, 32))
    n_all = 4099
    u = torch.from_numpy(uniform(n_all, seed=9)).cuda()

    def run(ut, active=None):
        ds, w = c.seq.sample_direction(None, ut, c.lam, active=active)
        return [host(x) for x in (ds.d, ds.pdf, w, c.seq.pdf_direction(None, ds, active=active))]

    full = run(u)
    assert np.any(full[1] > 0) and np.any(full[2] != 0)
    e = run(u[:, :0])
    assert e[0].shape == (3, 0) and e[1].shape == (0,) and e[3].shape == (0,)
    for n in range(1, 8):
        for lo in (0, 1, 4092):
            flat = torch.empty(2 * n + 1, device="cuda")   # planes 4 bytes off any 16-byte boundary
            un = flat[1:].view(2, n)
            un.copy_(u[:, lo:lo + n])
            assert un.data_ptr() % 16 == 4
            for got, ref in zip(run(un), full):
                np.testing.assert_array_equal(got, ref[..., lo:lo + n])
    mask = torch.from_numpy((np.arange(n_all) % 2).astype(np.uint8)).cuda()
    d, pdf, w, p = run(u, mask)
    np.testing.assert_array_equal(d, full[0])
    assert np.all(pdf[::2] == 0) and np.all(w[:, ::2] == 0) and np.all(p[::2] == 0)
    for got, ref in zip((pdf, w, p), full[1:]):
        np.testing.assert_array_equal(got[..., 1::2], ref[..., 1::2])
    # it.p moves ds.p and ds.dist only
    itp = torch.from_numpy(np.random.default_rng(3).normal(size=(3, n_all)).astype(np.float32)).cuda()
    ds, w2 = c.seq.sample_direction(ss.Interaction3f(p=itp), u, c.lam)
    np.testing.assert_array_equal(host(ds.d), full[0])
    np.testing.assert_array_equal(host(w2), full[2])
    inf = c.parent.info()
    rel = host(itp).astype(np.float64) - np.asarray(inf["bsphere_center"], np.float64)[:, None]
    dist = 2 * np.maximum(inf["bsphere_radius"], np.linalg.norm(rel, axis=0))
    np.testing.assert_allclose(host(ds.dist), dist, rtol=1e-6)
    np.testing.assert_allclose(host(ds.p), host(itp) + full[0] * host(ds.dist), rtol=1e-5, atol=1e-5)


def test_a_grid_smaller_than_the_work_is_bitwise_the_default_grid(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 walks the grid-stride loops two to three
    times per lane; this process makes the same calls at the default grid (one step)."""
    n = W.batch_size()
    env = dict(os.environ, SUNSKY_AMD_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, W.__file__, str(n), str(tmp_path)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    for variant, precision in W.COMBOS:
        child = np.load(tmp_path / f"{variant}_{precision}.npz")
        mine = W.run(variant, precision, n)
        for key in ("d", "pdf", "w", "p"):
            assert child[key].shape == mine[key].shape and np.any(mine[key] != 0)
            np.testing.assert_array_equal(child[key], mine[key])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_identity_code_object_gives_the_general_ones_bits(variant, precision, monkeypatch):
    s = samples(variant, precision, False)
    monkeypatch.setenv("SUNSKY_AMD_GENERAL_XFORM", "1")
    ds, w = s.c.seq.sample_direction(None, torch.from_numpy(s.u).cuda(), s.c.lam)
    p = s.c.seq.pdf_direction(None, ds)
    for got, ref in ((ds.d, s.d), (ds.pdf, s.pdf), (w, s.w), (p, s.p)):
        np.testing.assert_array_equal(host(got), ref)


# ---------------------------------------------------------------- 9. graph capture
@pytest.mark.parametrize("variant", VARIANTS)
def test_sampling_replays_bitwise_from_a_graph(variant):
    """sample_direction + pdf_direction captured once on a side stream and replayed twice: the
    outputs equal the direct calls bit for bit; nothing is allocated between capture and replay."""
    s = samples(variant, "fast", False)
    L, n = ss.lib(), s.u.shape[1]
    u = torch.from_numpy(s.u).cuda()
    nw = s.w.shape[0]
    d, pos = torch.zeros((3, n), device="cuda"), torch.zeros((3, n), device="cuda")
    pdf, dist, p, w = (torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"),
                       torch.zeros((nw, n), device="cuda"))
    from sunsky_amd import _capi
    import ctypes as C
    lam = (C.c_float * len(s.c.lam))(*s.c.lam) if s.c.lam else None
    m = len(s.c.lam) if s.c.lam else 0
    v3o = lambda t: _capi.Vec3Out(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())   # noqa: E731

    def calls():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.sunsky_sequence_sample_direction(s.c.seq._h, u[0].data_ptr(), u[1].data_ptr(), _capi.Vec3In(None, None, None),
                                                  lam, m, None, n, v3o(d), pdf.data_ptr(), dist.data_ptr(), v3o(pos),
                                                  w.data_ptr(), n, st) == 0
        assert L.sunsky_sequence_pdf_direction(s.c.seq._h, _capi.Vec3In(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr()),
                                               None, n, p.data_ptr(), st) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls()
    allocated = torch.cuda.memory_allocated()
    for _ in range(2):
        for t in (d, pdf, p, w):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, ref in ((d, s.d), (pdf, s.pdf), (w, s.w), (p, s.p)):
            np.testing.assert_array_equal(got.cpu().numpy(), ref)
    assert torch.cuda.memory_allocated() == allocated


# ---------------------------------------------------------------- 10. K = 1
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_frame_against_its_single_emitter(variant, precision):
    """K = 1, w = 1: the sun-pick pdf term is the emitter's sun_pdf, and the weight's numerator is
    the single emitter's eval at the sampled directions bit for bit (sequence.eval at K = 1 is the
    emitter's), so weight x pdf equals it to the rounding of the quotient."""
    s = samples(variant, precision, False, "one", (16, 32))
    r, c = s.c.ref, s.c
    assert c.K == 1 and r.q[0] == 1.0
    em = ss.SunskyEmitter(frame_dict(c.base, c.dirs[0], c.turb[0]), variant, precision=precision)
    wi = torch.from_numpy(-s.d).cuda()
    ev = host(em.eval(ss.SurfaceInteraction3f(wi=wi)) if c.lam is None else em.eval_spectral_broadcast(wi, c.lam))
    np.testing.assert_array_equal(s.e, ev)
    sun = s.u[0] >= r.w_sky
    hit, edge = r.cone_hits(s.local)
    assert sun.sum() > 100 and np.all(hit[sun & ~edge, 0])
    row, col, _ = r.cells(s.local)
    sky_term = float(r.w_sky) * r.f[row, col].astype(np.float64) / (r.S * r.omega)
    sun_term = (s.pdf.astype(np.float64) - sky_term)[sun & ~edge & (s.pdf > 0)] / (1.0 - float(r.w_sky))
    sun_pdf = 0.15915494309189533577 / (1.0 - float(r.cos_cutoff))
    print(f"sun-pick pdf term / sun_pdf - 1: {np.abs(sun_term / sun_pdf - 1).max():.3e}")
    assert np.abs(sun_term / sun_pdf - 1).max() <= 1e-5
    act = s.pdf > 0
    if precision == "reference":   # weight = eval / pdf, the IEEE quotient
        np.testing.assert_array_equal(s.w[:, act], ev[:, act] / s.pdf[act][None, :])
    assert rel_err(s.w[:, act].astype(np.float64) * s.pdf[act], ev[:, act]).max() <= 1e-5
