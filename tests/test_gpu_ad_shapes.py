"""The AD kernels (sunsky_eval_jvp_rgb / _spec, sunsky_eval_vjp_rgb / _spec, sunsky_grad_reduce)
at every launch shape and input edge they have a path for.  tests/test_eval_jvp.py holds them
to their bars at one shape: 17,408 rays = 68 full workgroups, no mask, 4 wavelength planes
inside (330, 710).  Here:

A. forward mode per lane: tiny and empty batches, 1 / 3 / 4 / 16 wavelength planes, wavelengths
   on the nodes, at both ends, out of range and NaN, and the `active` mask;
C. reverse mode at every shape of its two reductions: a ragged last workgroup, idle waves,
   sunsky_grad_reduce's unrolled loop (16 loads in flight while b + 240 < nblocks) with its
   hand-off to the remainder loop, and a batch beyond the VJP's own grid of
   min(ceil(n / 256), 6 x CUs) workgroups (sunsky_eval_vjp, csrc/sunsky_launch.h), where some
   lanes take a second grid-stride step; each against the JVP prefix sums, and bit for bit
   with a cotangent on one lane only, which no bar can hide a lost workgroup behind;
D. reverse mode with a mask and at the wavelength edges;
E. reverse mode against finite differences of the fp64 oracle, which shares nothing with the
   forward kernels or with the tangent staging both modes read.
(B, the forward mode over more than one grid-stride step, is in tests/test_gpu_grid_stride.py.)

Two references, no new tolerance:
1. per-lane contributions of one JVP sweep, C[p][i] = sum_k cot[k, i] dval_p[k, i] in fp64 on
   the host: the gradient of a prefix of m rays is C[p][:m].sum() with magnitude
   |C[p][:m]|.sum(), held to test_eval_jvp._vjp_vs_jvp's bar, 1e-4 mag + 1e-12.  One sweep at
   the largest batch serves every prefix because a lane's JVP does not depend on the batch
   size (shown bitwise in A);
2. 4-point central differences of the fp64 oracle at the steps test_eval_jvp.py uses (1e-3 for
   turbidity and albedo, 1e-4 along tangents orthogonal to the sun), held to check() per lane
   and to 1e-3 of the contraction's magnitude for the VJP (the sun-disc test's bar).
Every test prints its worst ratio to the bar it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

import oracle as O
import sunsky_amd as ss
from helpers import assert_parity, hemisphere_wo, sun_cone_wo
from test_eval_jvp import _gpu, check, rays, scene

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
NODES = np.arange(320, 721, 40, dtype=np.float32)                    # the 11 model wavelengths
OUT_OF_RANGE = np.array([319.99, 720.01, -1.0, 1e9, np.nan], np.float32)
N_SMALL = 4099
EDGE_SIZES = [0, 1, 2, 3, 5, 7, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _nch(variant):
    return 11 if variant == "spectral" else 3


def _si(wi, lam=None):
    return ss.SurfaceInteraction3f(wi=wi, wavelengths=lam)


def _head(x, m):
    return None if x is None else x[..., :m].contiguous()


def _same_bits(a, b):
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _basis(variant):
    """(index in grad, parameter, basis tangent) of the 15 gradients eval_vjp accumulates."""
    nch = _nch(variant)
    return ([(0, "turbidity", [1.0])] + [(1 + c, "albedo", list(np.eye(nch)[c])) for c in range(nch)]
            + [(12 + a, "sun_direction", list(np.eye(3)[a])) for a in range(3)])


def _tangents(variant):
    """One tangent of each differentiable parameter."""
    return [("turbidity", [1.0]), ("albedo", list(np.linspace(0.5, 1.5, _nch(variant)))),
            ("sun_direction", [0.3, -0.2, 0.5])]


def _contributions(em, variant, si, cot):
    """Reference 1: (16, n) fp64, row p = the per-lane contributions to grad[p] from eval_jvp
    along p's basis tangent, contracted with `cot` ((k, n) fp64) on the host.  Rows no
    parameter owns (RGB albedo channels 3..10, and 15) stay 0: eval_vjp must leave 0 there."""
    c = np.zeros((16, cot.shape[1]))
    for idx, param, tan in _basis(variant):
        dv = em.eval_jvp(si, param, tan)[1].cpu().numpy().astype(np.float64)
        c[idx] = (cot * dv).sum(axis=0)
    return c


def _hold_to_contributions(grad, c, what):
    """|grad[p] - sum C[p]| <= 1e-4 sum |C[p]| + 1e-12 for all 16 entries (_vjp_vs_jvp's bar);
    grad[15] exactly 0.  Returns the worst ratio to the bar."""
    g = grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), (what, g)
    assert g[15] == 0.0, (what, g[15])
    ref, mag = c.sum(axis=1), np.abs(c).sum(axis=1)
    ratio = np.abs(g - ref) / (1e-4 * mag + 1e-12)
    print(f"{what}: VJP vs JVP prefix sums, worst {ratio.max():.2e} of the 1e-4 bar (grad[{int(ratio.argmax())}])")
    assert (ratio <= 1.0).all(), (what, [(p, g[p], ref[p], mag[p]) for p in np.nonzero(ratio > 1.0)[0]])
    return float(ratio.max())


def _check_ratio(jvp, fd, mask):
    """Worst ratio to check()'s bound, 2e-3 |fd| + 1e-4 max |fd|."""
    f = fd[mask]
    return float(np.max(np.abs(jvp[mask].astype(np.float64) - f) / (2e-3 * np.abs(f) + 1e-4 * np.abs(f).max())))


# ---------------------------------------------------------------- reference 2: fp64 finite differences
def _oracle_planes(d, variant, wi, lam):
    """fp64 oracle eval as (k, n) planes, like the kernels' outputs."""
    v = O.Oracle(d, variant, "jit", "f64").eval(wi, lam if variant == "spectral" else None)
    return v if variant == "spectral" else v.T.copy()


def _d4(f, h, s):
    """4-point central difference at step s h of the samples f[k] taken at offset k h."""
    return (8.0 * (f[s] - f[-s]) - (f[2 * s] - f[-2 * s])) / (12.0 * s * h)


def _fd(variant, wi, lam, at, h, coarse=True):
    """at(x) -> (scene dict at offset x along the tangent, the parameter values the oracle then
    sees).  The oracle takes its parameters in fp32, so the points it is given are offsets
    k h rounded to fp32 (up to 1.2e-4 of a step of 1e-3 at turbidity 3.4); differencing the
    points with the stencil's own weights gives the tangent the differences were really taken
    along, and the derivative is linear in it.  -> (d, tangent) at step h and, with `coarse`,
    the same stencil at 2 h."""
    f, p = {}, {}
    for k in ((-4, -2, -1, 1, 2, 4) if coarse else (-2, -1, 1, 2)):
        d, p[k] = at(k * h)
        f[k] = _oracle_planes(d, variant, wi, lam)
    return [(_d4(f, h, s), _d4(p, h, s)) for s in ((1, 2) if coarse else (1,))]


def _at_turbidity(d):
    def at(x):
        t = np.float32(d["turbidity"] + x)
        return dict(d, turbidity=float(t)), np.float64(t)
    return at


def _at_albedo(d, variant, channels):
    base = O.albedo_values(d["albedo"], variant == "spectral")

    def at(x):
        a = base.copy()
        a[channels] = (base[channels].astype(np.float64) + x).astype(np.float32)
        return dict(d, albedo=[float(v) for v in a]), a[channels].astype(np.float64)
    return at


def _at_sun(d, t):
    s = np.array(d["sun_direction"], np.float64)
    s /= np.linalg.norm(s)

    def at(x):
        v = ((s + x * t) / np.linalg.norm(s + x * t)).astype(np.float32)
        u = v.astype(np.float64)
        return dict(d, sun_direction=[float(c) for c in v]), u / np.linalg.norm(u)
    return at


def _sun_tangents(d):
    s = np.array(d["sun_direction"], np.float64)
    s /= np.linalg.norm(s)
    t1 = np.cross(s, [0.0, 0.0, 1.0])
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(s, t1)


H_SCALAR, H_SUN = 1e-3, 1e-4   # tests/test_eval_jvp.py's steps


def fd_gradient_reference(d, variant, wi, lam, cot, cot_sun):
    """Reference 2 for the reverse mode, CPU only: for turbidity, every albedo channel and two
    sun tangents orthogonal to the sun, rows (label, "all" | "sky": which cotangent, weights w
    with the expected value of w . grad, sum cot FD at step h, the same at 2 h, sum |cot FD|).
    wi (n, 3), lam and the cotangents (k, n); cot_sun is zero on the lanes within 1 degree of
    the sun too.  The sun axes take cot_sun alone; turbidity and albedo take both, because the
    disc lanes carry 1e3 times the sky's turbidity derivative and own the magnitude of the
    "all" rows: the "sky" rows hold the sky lanes to a bar of their own size.

    Spectral albedo: a lane's plane reads the two channels around its wavelength, lo and
    lo + 1, and channel c's tables depend on albedo[c] alone (compute_radiance_params,
    sunsky.h:158-231), so stepping all even channels at once gives every plane the derivative
    along its one even channel, likewise the odd ones: 2 oracle sweeps instead of 11."""
    nch = _nch(variant)
    rows = []

    def row(label, w, d1, d2, which=("all", "sky")):
        for name in which:
            c = cot if name == "all" else cot_sun
            rows.append((label, name, w, float((c * d1).sum()), float((c * d2).sum()), float(np.abs(c * d1).sum())))

    def unit(idx):
        w = np.zeros(16)
        w[idx] = 1.0
        return w

    (d1, s1), (d2, s2) = _fd(variant, wi, lam, _at_turbidity(d), H_SCALAR)
    row("turbidity", unit(0), d1 / s1, d2 / s2)
    if variant == "spectral":
        lo = np.floor((lam.astype(np.float64) - 320.0) / 40.0).astype(int)
        for parity in (0, 1):
            ch = np.arange(parity, nch, 2)
            (d1, s1), (d2, s2) = _fd(variant, wi, lam, _at_albedo(d, variant, ch), H_SCALAR)
            mine = np.where(lo % 2 == parity, lo, lo + 1)       # the plane's channel of this parity
            for j, c in enumerate(ch):
                sel = mine == c
                row(f"albedo[{c}]", unit(1 + c), np.where(sel, d1, 0.0) / s1[j], np.where(sel, d2, 0.0) / s2[j])
    else:
        for c in range(nch):
            (d1, s1), (d2, s2) = _fd(variant, wi, lam, _at_albedo(d, variant, np.array([c])), H_SCALAR)
            row(f"albedo[{c}]", unit(1 + c), d1 / s1[0], d2 / s2[0])
    for name, t in zip(("t1", "t2"), _sun_tangents(d)):
        (d1, s1), (d2, s2) = _fd(variant, wi, lam, _at_sun(d, t), H_SUN)
        w = np.zeros(16)
        w[12:15] = s1        # the tangent the step-h differences were taken along
        row(f"sun_direction.{name}", w, d1, d2, which=("sky",))
    return rows


def assert_stencils_agree(rows):
    """The reference's own error, shown: the 4-point stencil at h against the same stencil at
    2 h, whose truncation error is 16 times larger and whose rounding noise is half.  They
    must agree within a tenth of the VJP bar (1e-4 of the magnitude), which leaves nine tenths
    of the bar to the kernels.  Returns the worst ratio to that tenth."""
    worst = 0.0
    for label, which, _, r1, r2, mag in rows:
        assert mag > 0.0, (label, which)
        ratio = abs(r1 - r2) / (1e-4 * mag)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (label, which, r1, r2, mag)
    return worst


# ---------------------------------------------------------------- A. forward mode, per lane
@functools.lru_cache(maxsize=None)
def _small(variant):
    """N_SMALL rays: a hemisphere with every fourth lane inside the sun disc, so that disc
    lanes sit in the shortest prefixes too; 16 wavelength planes in (330, 710)."""
    d = scene()
    em = ss.load_dict(d, variant=variant)
    o32 = O.Oracle(d, variant, "jit", "f32")
    inf = o32.info()
    wo = hemisphere_wo(N_SMALL, seed=31)
    wo[::4] = sun_cone_wo(len(wo[::4]), inf["sun_dir_local"], np.arccos(inf["cos_cutoff"]), seed=32, scale=0.9)
    lam = np.random.default_rng(33).uniform(330, 710, (16, N_SMALL)).astype(np.float32)
    sun = (wo.astype(np.float64) @ inf["sun_dir_local"] >= inf["cos_cutoff"]) & (wo[:, 2] >= 0)
    assert sun[0] and sun.sum() >= N_SMALL // 5
    return dict(d=d, em=em, o32=o32, wo=wo, wi=_gpu(-wo), sun=sun,
                lam=torch.from_numpy(lam).cuda() if variant == "spectral" else None)


def _edge_planes(n):
    """(4, n) wavelength planes: (a) the 11 nodes cycled over the lanes (f == 0, no upper
    channel), (b) 720 exactly (lo = 10, hi = 11 is outside the table) and the fp32 just below
    it, (c) 320 exactly, (d) out of range and NaN."""
    i = np.arange(n)
    below = np.nextafter(np.float32(720.0), np.float32(0.0))
    return np.stack([NODES[i % 11], np.where(i % 2 == 0, np.float32(720.0), below),
                     np.full(n, 320.0, np.float32), OUT_OF_RANGE[i % len(OUT_OF_RANGE)]]).astype(np.float32)


@pytest.mark.parametrize("variant", VARIANTS)
def test_jvp_tiny_and_empty_batches_match_the_large_batch(variant):
    """eval_jvp of the first k rays gives the bits of the first k lanes of the full batch, val
    and dval, for a tangent of each parameter; k = 0 returns empty tensors."""
    s = _small(variant)
    em = s["em"]
    lam = s["lam"][:4].contiguous() if variant == "spectral" else None
    for param, tan in _tangents(variant):
        full = em.eval_jvp(_si(s["wi"], lam), param, tan)
        for k in EDGE_SIZES:
            part = em.eval_jvp(_si(_head(s["wi"], k), _head(lam, k)), param, tan)
            for name, a, b in zip(("val", "dval"), part, full):
                assert a.shape == (b.shape[0], k), (param, k, name, tuple(a.shape))
                assert _same_bits(a, b[:, :k]), f"{param} k={k} {name} differs from the large batch"
    torch.cuda.synchronize()


@pytest.mark.parametrize("nlam", [1, 3, 4, 16])
def test_jvp_spectral_plane_counts(nlam):
    """Plane q of an nlam-plane call equals the single-plane call on that plane's wavelengths."""
    s = _small("spectral")
    em = s["em"]
    for param, tan in _tangents("spectral"):
        val, dval = em.eval_jvp(_si(s["wi"], s["lam"][:nlam].contiguous()), param, tan)
        assert val.shape == dval.shape == (nlam, N_SMALL)
        for q in range(nlam):
            v1, d1 = em.eval_jvp(_si(s["wi"], s["lam"][q:q + 1].contiguous()), param, tan)
            assert _same_bits(val[q], v1[0]) and _same_bits(dval[q], d1[0]), (param, nlam, q)


def test_jvp_spectral_wavelength_edges_against_the_oracle():
    """Wavelengths on the nodes, at 720 / just below / 320: val to the oracles by assert_parity,
    dval to fp64 finite differences by check(), for turbidity and albedo.  Out of range and
    NaN: val and dval exactly 0, for every parameter."""
    s = _small("spectral")
    em, d, wo = s["em"], s["d"], s["wo"]
    lam = _edge_planes(N_SMALL)
    si = _si(s["wi"], torch.from_numpy(lam).cuda())
    for param, tan in _tangents("spectral"):
        val, dval = em.eval_jvp(si, param, tan)
        assert bool((val[3] == 0).all()) and bool((dval[3] == 0).all()), param
    inside = lam[:3]
    ref32 = s["o32"].eval(-wo, inside).T
    ref64 = O.Oracle(d, "spectral", "jit", "f64").eval(-wo, inside).T
    lanes = (wo[:, 2] > 1e-3)[None, :].repeat(3, 0)   # finite differences straddle no horizon
    for param, at in (("turbidity", _at_turbidity(d)), ("albedo", _at_albedo(d, "spectral", np.arange(11)))):
        val, dval = em.eval_jvp(si, param, [1.0])
        assert_parity(val[:3].cpu().numpy().T, ref32, ref64, s["sun"], precision="reference")
        (fd, step), = _fd("spectral", -wo, inside, at, H_SCALAR, coarse=False)
        fd = fd / np.atleast_1d(step)[0]
        dv = dval[:3].cpu().numpy()
        assert np.abs(fd[lanes]).max() > 0
        print(f"{param} at the wavelength edges: JVP vs FD worst {_check_ratio(dv, fd, lanes):.2e} of check()'s bound")
        check(dv, fd, lanes)


@pytest.mark.parametrize("variant", VARIANTS)
def test_jvp_mask(variant):
    """Masked lanes, with NaN directions and wavelengths, give exactly 0; the others give the
    bits of the unmasked call on clean inputs.  Also an all-false mask and active=False."""
    s = _small(variant)
    em, wi = s["em"], s["wi"]
    lam = s["lam"][:4].contiguous() if variant == "spectral" else None
    on = torch.from_numpy(np.random.default_rng(34).random(N_SMALL) < 0.5).cuda()
    assert 0.4 < float(on.float().mean()) < 0.6
    wi_p = wi.clone()
    wi_p[:, ~on] = float("nan")
    lam_p = None
    if lam is not None:
        lam_p = lam.clone()
        lam_p[:, ~on] = float("nan")
    for param, tan in _tangents(variant):
        clean = em.eval_jvp(_si(wi, lam), param, tan)
        got = em.eval_jvp(_si(wi_p, lam_p), param, tan, active=on)
        for name, a, b in zip(("val", "dval"), got, clean):
            assert bool((a[:, ~on] == 0).all()), f"{param} {name}: a masked lane is not 0"
            assert _same_bits(a[:, on], b[:, on]), f"{param} {name}: an unmasked lane differs"
        for off in (torch.zeros(N_SMALL, dtype=torch.bool, device="cuda"), False):
            for a in em.eval_jvp(_si(wi_p, lam_p), param, tan, active=off):
                assert bool((a == 0).all()), (param, off)


# ---------------------------------------------------------------- C. reverse mode, every shape of the reduction
def _big_n():
    return 6 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 773


# (id, m given N): what the prefix of m rays exercises
PREFIXES = [
    ("1_one_lane", lambda n: 1),
    ("63_inside_a_wave", lambda n: 63),
    ("64_one_full_wave", lambda n: 64),
    ("65_second_wave_one_lane", lambda n: 65),
    ("255_ragged_workgroup", lambda n: 255),
    ("256_one_workgroup", lambda n: 256),
    ("257_ragged_second_workgroup", lambda n: 257),
    ("17408_68_full_workgroups", lambda n: 17408),
    ("240x256_last_grid_with_no_unrolled_iteration", lambda n: 240 * 256),
    ("240x256+1_segment_0_alone_unrolled", lambda n: 240 * 256 + 1),
    ("241x256+1_segments_0_and_1_unrolled", lambda n: 241 * 256 + 1),
    ("250x256-5_some_segments_unrolled", lambda n: 250 * 256 - 5),
    ("258x256-5_all_unrolled_once_remainder_in_two", lambda n: 258 * 256 - 5),
    ("513x256+3_two_unrolled_iterations", lambda n: 513 * 256 + 3),
    ("N_second_grid_stride_step", lambda n: n),
]


def _tiled_dirs(o32, n, seed):
    """rays()-style blocks (16,384 hemisphere + 1,024 sun-cone directions) with a new seed per
    block, then one fixed shuffle: about 6 % disc lanes in every prefix, short ones included."""
    inf = o32.info()
    half = np.arccos(inf["cos_cutoff"])
    blocks, have, s = [], 0, seed
    while have < n:
        blocks += [hemisphere_wo(1 << 14, seed=s), sun_cone_wo(1024, inf["sun_dir_local"], half, seed=s + 1, scale=0.9)]
        have += (1 << 14) + 1024
        s += 2
    wo = np.concatenate(blocks)[:n]
    return np.ascontiguousarray(wo[np.random.default_rng(seed).permutation(n)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _big(variant):
    """N = 6 x 256 x CUs + 773 rays, a random cotangent, and reference 1 from one JVP sweep at N."""
    n = _big_n()
    d = scene()
    em = ss.load_dict(d, variant=variant)
    wo = _tiled_dirs(O.Oracle(d, variant, "jit", "f32"), n, seed=41)
    rng = np.random.default_rng(42)
    k = 4 if variant == "spectral" else 3
    lam = torch.from_numpy(rng.uniform(330, 710, (4, n)).astype(np.float32)).cuda() if variant == "spectral" else None
    cot = rng.standard_normal((k, n)).astype(np.float32)
    wi = _gpu(-wo)
    c = _contributions(em, variant, _si(wi, lam), cot.astype(np.float64))
    return dict(n=n, em=em, wi=wi, lam=lam, cot=torch.from_numpy(cot).cuda(), cot_host=cot, c=c)


def _vjp_prefix(em, b, m, **kw):
    return em.eval_vjp(_si(_head(b["wi"], m), _head(b["lam"], m)), _head(b["cot"], m), **kw)[0]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("prefix", [p[1] for p in PREFIXES], ids=[p[0] for p in PREFIXES])
def test_vjp_prefix_holds_to_the_jvp_prefix_sums(variant, prefix):
    b = _big(variant)
    m = prefix(b["n"])
    assert 1 <= m <= b["n"], (m, b["n"])
    grad = _vjp_prefix(b["em"], b, m)
    _hold_to_contributions(grad, b["c"][:, :m], f"{variant} m={m}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_vjp_empty_batch_leaves_grad_untouched(variant):
    b = _big(variant)
    grad = torch.arange(16, dtype=torch.float32, device="cuda") + 0.5
    before = grad.clone()
    out = _vjp_prefix(b["em"], b, 0, grad=grad)
    torch.cuda.synchronize()
    assert out is grad and _same_bits(grad, before)


@pytest.mark.parametrize("variant", VARIANTS)
def test_vjp_deterministic_and_accumulating_beyond_one_grid(variant):
    """At N (some lanes take two grid-stride steps): two calls give equal bits, and a call with
    grad= adds (2 x grad at rtol 1e-6, as test_eval_vjp_matches_jvp_contractions)."""
    b = _big(variant)
    g1 = _vjp_prefix(b["em"], b, b["n"])
    g2 = _vjp_prefix(b["em"], b, b["n"])
    assert _same_bits(g1, g2)
    _vjp_prefix(b["em"], b, b["n"], grad=g2)
    assert torch.allclose(g2, 2 * g1, rtol=1e-6, atol=0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_vjp_small_batch_after_a_large_one(variant):
    """After a call at N the emitter's partials buffer is larger than the next call's grid and
    holds that call's sums past nblocks: a call at m = 65 gives the bits of a fresh emitter's."""
    b = _big(variant)
    _vjp_prefix(b["em"], b, b["n"])
    after = _vjp_prefix(b["em"], b, 65)
    fresh = _vjp_prefix(ss.load_dict(scene(), variant=variant), b, 65)
    assert _same_bits(after, fresh), (after, fresh)
    assert bool((after[:1] != 0).all())


# (m given N, lanes given m and N): lanes whose sums reach grad through each path
ONE_HOT = [
    (lambda n: 65, lambda m, n: [0, 63, 64]),                      # wave 0, and the one lane of wave 1
    (lambda n: 257, lambda m, n: [255, 256]),                      # the one lane of a ragged workgroup
    # nblocks = 250: segments 0 .. 9 unrolled (block 5 a first load, block 249 a last one), segment 10 not
    # (blocks 10 .. 234)
    (lambda n: 250 * 256 - 5, lambda m, n: [5 * 256 + 17, 249 * 256 + 250, 10 * 256, 234 * 256 + 1, 240 * 256]),
    # nblocks = 258: all unrolled once, then blocks 256 and 257 in the remainder loop
    (lambda n: 258 * 256 - 5, lambda m, n: [15 * 256, 255 * 256 + 9, 256 * 256, m - 1]),
    # nblocks = 514: segment 0 takes blocks 0, 16 .. 240, then 256 .. 496, then 512
    (lambda n: 513 * 256 + 3, lambda m, n: [17 * 256, 256 * 256 + 1, 496 * 256 + 3, 512 * 256, m - 1]),
    # N: the grid is 6 x CUs workgroups; lanes N - 773 .. N - 1 are second grid-stride steps
    (lambda n: n, lambda m, n: [0, 772, 773, n - 773 - 1, n - 773, n - 1]),
]


@pytest.mark.parametrize("variant", VARIANTS)
def test_vjp_one_lane_cotangent_reaches_grad_through_every_path(variant):
    """With a cotangent that is zero on every lane but j, every other lane adds an exact zero
    in its own accumulators, in the wave shuffles, in LDS, in the partials and in
    sunsky_grad_reduce: the gradient has the bits of the call on lane j alone, wherever j's
    workgroup sits in the reduction.  A partial that is dropped, read twice or read stale
    shows here whatever its size; the 1e-4 bar of the prefix sums would hide one workgroup
    among hundreds."""
    b = _big(variant)
    em = b["em"]
    for m_of, lanes_of in ONE_HOT:
        m = m_of(b["n"])
        wi, lam = _head(b["wi"], m), _head(b["lam"], m)
        for j in lanes_of(m, b["n"]):
            assert 0 <= j < m
            cot = torch.zeros((b["cot"].shape[0], m), device="cuda")
            cot[:, j] = b["cot"][:, j]
            hot = em.eval_vjp(_si(wi, lam), cot)[0]
            one = em.eval_vjp(_si(wi[:, j:j + 1].contiguous(), None if lam is None else lam[:, j:j + 1].contiguous()),
                              b["cot"][:, j:j + 1].contiguous())[0]
            assert bool(one[0] != 0), (m, j)
            assert _same_bits(hot, one), (variant, m, j, hot, one)


# ---------------------------------------------------------------- D. reverse mode: mask and wavelength edges
@pytest.mark.parametrize("variant", VARIANTS)
def test_vjp_mask(variant):
    """m = 258 x 256 - 5, a random mask, NaN directions / cotangents / wavelengths on the masked
    lanes: a finite gradient that holds to the contributions of the unmasked lanes alone.  An
    all-false mask leaves grad untouched."""
    b = _big(variant)
    em, m = b["em"], 258 * 256 - 5
    on_host = np.random.default_rng(43).random(m) < 0.5
    on = torch.from_numpy(on_host).cuda()
    nan = float("nan")
    wi, cot, lam = _head(b["wi"], m), _head(b["cot"], m), _head(b["lam"], m)
    wi[:, ~on] = nan
    cot[:, ~on] = nan
    if lam is not None:
        lam[:, ~on] = nan
    grad = em.eval_vjp(_si(wi, lam), cot, active=on)[0]
    _hold_to_contributions(grad, b["c"][:, :m][:, on_host], f"{variant} m={m} masked")
    pre = torch.arange(16, dtype=torch.float32, device="cuda") - 3.25
    before = pre.clone()
    for off in (torch.zeros(m, dtype=torch.bool, device="cuda"), False):
        em.eval_vjp(_si(wi, lam), cot, active=off, grad=pre)
        assert _same_bits(pre, before), off


@pytest.mark.parametrize("rows", [[0], [1, 2, 3], list(range(16))], ids=["1_plane", "3_planes", "16_planes"])
def test_vjp_spectral_wavelength_edges(rows):
    """The edge planes of the forward test (nodes; 720 and just below; 320; out of range and
    NaN) plus 12 planes in (330, 710), taken 1, 3 and 16 at a time: the gradient holds to the
    JVP contractions of the same call.  The out-of-range and NaN wavelengths carry a NaN
    cotangent and must contribute nothing."""
    s = _small("spectral")
    em = s["em"]
    lam = np.concatenate([_edge_planes(N_SMALL), s["lam"][4:].cpu().numpy()])[rows]
    valid = (lam >= 320.0) & (lam <= 720.0)      # NaN compares false
    assert valid.any() and (len(rows) == 1 or not valid.all())
    cot = np.random.default_rng(44).standard_normal(lam.shape).astype(np.float32)
    si = _si(s["wi"], torch.from_numpy(lam).cuda())
    grad = em.eval_vjp(si, torch.from_numpy(np.where(valid, cot, np.float32(np.nan))).cuda())[0]
    c = _contributions(em, "spectral", si, np.where(valid, cot, 0.0).astype(np.float64))
    _hold_to_contributions(grad, c, f"spectral edge planes {rows}")


def test_vjp_spectral_node_wavelength_reaches_one_albedo_channel():
    """Every lane exactly on node c (f == 0, the low channel only): the gradient of every other
    albedo channel is exactly 0."""
    s = _small("spectral")
    cot = torch.from_numpy(np.random.default_rng(45).standard_normal((1, N_SMALL)).astype(np.float32)).cuda()
    for c in range(11):
        lam = torch.full((1, N_SMALL), float(NODES[c]), device="cuda")
        g = s["em"].eval_vjp(_si(s["wi"], lam), cot)[0].cpu().numpy()
        others = np.delete(g[1:12], c)
        assert g[1 + c] != 0.0 and np.all(others == 0.0), (c, g[1:12])


# ---------------------------------------------------------------- E. reverse mode against the oracle
def fd_case(variant, case):
    """-> (scene, rotation): scene() or test_eval_vjp_sun_axes_across_elevations_and_frames's
    rotated frame, with distinct albedo values per channel."""
    rot = np.eye(3)
    if case == "rotated":
        d = scene(sun=[0.4, 0.3, 0.8])
        c, s = math.cos(0.7), math.sin(0.7)
        d["to_world"] = np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], np.float32)
        rot = d["to_world"][:3, :3].astype(np.float64)
    else:
        d = scene()
    d["albedo"] = [float(v) for v in np.linspace(0.15, 0.65, _nch(variant)).astype(np.float32)]
    return d, rot


def fd_batch(d, variant, rot):
    """17,408 + 37 rays (the last workgroup ragged): rays() in the emitter's frame, taken to the
    world, wavelengths and a cotangent.  The cotangent is 0 where the differences are not
    valid: wo_z <= 1e-3 in the emitter's frame (they would straddle the horizon) and, for the
    sun axes, within 1 degree of the sun (the disc test flips, d gamma is singular at 0; that
    part is held by test_sun_disc_tangent_along_sun_direction)."""
    o32 = O.Oracle(d, variant, "jit", "f32")
    local = np.concatenate([rays(o32), hemisphere_wo(37, seed=13)]).astype(np.float64)
    wo = (local @ rot.T).astype(np.float32)
    n = wo.shape[0]
    assert n == 17408 + 37 and n % 256 != 0
    rng = np.random.default_rng(51)
    k = 4 if variant == "spectral" else 3
    lam = rng.uniform(330, 710, (4, n)).astype(np.float32)
    cot = rng.standard_normal((k, n)).astype(np.float32)
    s = np.array(d["sun_direction"], np.float64)
    s /= np.linalg.norm(s)
    horizon = (wo.astype(np.float64) @ rot)[:, 2] <= 1e-3
    near = wo.astype(np.float64) @ s >= math.cos(math.radians(1.0))
    assert near.sum() >= 1024 and (horizon | near).mean() <= 0.10, (horizon.mean(), near.mean())
    return wo, lam, cot * ~horizon, cot * ~(horizon | near)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", ["default", "rotated"])
def test_vjp_against_oracle_finite_differences(variant, case):
    """eval_vjp's turbidity, per-channel albedo and sun-axis gradients against sum cot FD of
    the fp64 oracle, to 1e-3 of the contraction's magnitude: a reference that shares neither
    the forward kernels nor sunsky_stage_tangent with the reverse mode."""
    d, rot = fd_case(variant, case)
    wo, lam, cot, cot_sun = fd_batch(d, variant, rot)
    rows = fd_gradient_reference(d, variant, -wo, lam, cot.astype(np.float64), cot_sun.astype(np.float64))
    print(f"{variant} {case}: stencil at h vs 2h, worst {assert_stencils_agree(rows):.2e} of a tenth of the bar")
    em = ss.load_dict(d, variant=variant)
    si = _si(_gpu(-wo), torch.from_numpy(lam).cuda() if variant == "spectral" else None)
    g = {"all": em.eval_vjp(si, torch.from_numpy(cot).cuda())[0].cpu().numpy().astype(np.float64),
         "sky": em.eval_vjp(si, torch.from_numpy(cot_sun).cuda())[0].cpu().numpy().astype(np.float64)}
    worst = {}
    for label, which, w, ref, _, mag in rows:
        got = float(w @ g[which])
        key = label.split("[")[0].split(".")[0] + " " + which
        worst[key] = max(worst.get(key, 0.0), abs(got - ref) / (1e-3 * mag))
        assert abs(got - ref) <= 1e-3 * mag, (label, which, got, ref, mag)
    print(f"{variant} {case}: VJP vs oracle FD, worst ratio to the 1e-3 bar", {k: f"{v:.2e}" for k, v in worst.items()})
