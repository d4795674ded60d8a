"""eval_jvp_dir / eval_vjp_dir / eval_wi: the derivative of eval(si) with respect to the ray
direction si.wi (sunsky_eval_{jvp,vjp}_dir_{rgb,spec}), RGB and spectral (4 wavelength planes,
random in 330..710).

Reference for the derivative tests: 4-point central differences of the fp64 oracle on the
sphere, tests/dir_ad_reference.py (which states the bar and why it is per lane gradient
magnitude).  Each of those tests first asserts that the oracle's own stencils at h and h / 2
agree to 0.1 (sky lanes) / 0.5 (sun-disc lanes) of the bar, then holds the kernel to the full
bar against the h stencil, and prints the worst ratios.

The other tests need no new tolerance: reverse against forward mode on the project's
VJP-vs-JVP bar (1e-4 of the summed magnitudes + 1e-12), the value against the oracles by
assert_parity as tests/test_eval_jvp.py holds eval_jvp's, and bitwise comparisons."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dir_ad_reference as R
import gpu_dir_ad_worker as W
import oracle as O
import sunsky_amd as ss
from helpers import assert_parity, hemisphere_wo, sun_cone_wo
from test_eval_jvp import _gpu, rays, scene

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
# (scene, to_world): the 40 deg / T 3.4 scene and a low sun with sky and disc lanes; a rotation
# and a non-orthonormal to_world with sky lanes (a missing M^-1 or a missing transpose shows)
CONFIGS = [("mid", "ident"), ("low", "ident"), ("mid", "rot"), ("mid", "scaled")]
CONFIG_IDS = [f"{s}_{x}" for s, x in CONFIGS]
OUT_OF_RANGE = np.array([319.99, 720.01, -1.0, 1e9, np.nan], np.float32)
N_SMALL = 4099
PREFIXES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4099]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _si(wi, lam=None):
    return ss.SurfaceInteraction3f(wi=wi, wavelengths=lam)


def _head(x, m):
    return None if x is None else x[..., :m].contiguous()


def _same_bits(a, b):
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _np64(t):
    return t.cpu().numpy().astype(np.float64)


def _lam(variant, lam):
    return torch.from_numpy(lam).cuda() if variant == "spectral" else None


@functools.lru_cache(maxsize=None)
def _emitter(scene_key, variant, xf):
    return ss.load_dict(R.scene_dict(scene_key, xf), variant=variant)


def _reference(scene_key, variant, xf):
    ref = R.reference(scene_key, variant, xf, xf == "ident")
    for group in ("sky", "disc"):
        if group in ref:
            R.assert_self_consistent(ref, group, f"{scene_key} {xf} {variant}")
    return ref


def _world(m, v):
    """Local directions / tangents (n, 3) -> the (3, n) device planes of wi = -to_world v."""
    return _gpu(-(v @ m.T))


# ---------------------------------------------------------------- 1, 2. forward mode vs FD
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
def test_jvp_dir_against_oracle_finite_differences(variant, config):
    """Per lane and channel, along two tangents of the sphere (and the radial one on sky lanes):
    d_wi = -to_world t gives d wo = t."""
    ref = _reference(config[0], variant, config[1])
    em = _emitter(config[0], variant, config[1])
    for group in ("sky", "disc"):
        if group not in ref:
            continue
        g = ref[group]
        si = _si(_world(ref["m"], g["wo"]), _lam(variant, g["lam"]))
        got = np.stack([_np64(em.eval_jvp_dir(si, _world(ref["m"], t))[1]) for t in g["dirs"]])
        assert np.isfinite(got).all()
        r = R.worst(got, g["fd"])
        print(f"{config} {variant} {group}: jvp_dir vs FD, worst {r:.3f} of the bar")
        assert r <= 1.0, (config, variant, group, r)


# ---------------------------------------------------------------- 3. reverse mode vs FD
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
def test_vjp_dir_against_oracle_finite_differences(variant, config):
    """grad_wi . d_wi_t against sum_c cot_c fd_t,c per lane, with a random cotangent, on the
    same bar applied to the contracted gradient."""
    ref = _reference(config[0], variant, config[1])
    em = _emitter(config[0], variant, config[1])
    for gi, group in enumerate(("sky", "disc")):
        if group not in ref:
            continue
        g = ref[group]
        k, n = g["fd"].shape[1:]
        cot = np.random.default_rng(80 + gi).standard_normal((k, n)).astype(np.float32)
        si = _si(_world(ref["m"], g["wo"]), _lam(variant, g["lam"]))
        grad = _np64(em.eval_vjp_dir(si, torch.from_numpy(cot).cuda()))
        assert grad.shape == (3, n) and np.isfinite(grad).all()
        d_wi = [-(t @ ref["m"].T).astype(np.float32).astype(np.float64) for t in g["dirs"]]
        got = np.stack([(grad * d.T).sum(axis=0) for d in d_wi])[:, None, :]
        fd = (cot.astype(np.float64)[None] * g["fd"]).sum(axis=1, keepdims=True)
        r = R.worst(got, fd)
        print(f"{config} {variant} {group}: vjp_dir vs FD, worst {r:.3f} of the bar")
        assert r <= 1.0, (config, variant, group, r)


# ---------------------------------------------------------------- 4. adjointness
def _horizon_wo(n, seed):
    """Unit directions with cos theta in [0, 0.02] (every eighth below the horizon)."""
    rng = np.random.default_rng(seed)
    ct = rng.uniform(0.0, 0.02, n)
    ct[::8] = -ct[::8] - 1e-3
    ct[1] = 0.0
    ph = rng.uniform(0, 2 * np.pi, n)
    st = np.sqrt(1 - ct * ct)
    return np.stack([st * np.cos(ph), st * np.sin(ph), ct], 1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
def test_vjp_dir_is_the_adjoint_of_jvp_dir(variant, config):
    """Per lane, sum_c cot_c jvp_dir(d_wi)_c = grad_wi . d_wi for random d_wi (not restricted to
    the tangent plane), to 1e-4 of the summed magnitudes of the terms of both contractions
    + 1e-12: sky, sun-disc and horizon-adjacent lanes."""
    ref = R.reference(config[0], variant, config[1], config[1] == "ident")
    em = _emitter(config[0], variant, config[1])
    inf = O.Oracle(ref["d"], variant, "jit", "f32").info()
    disc = sun_cone_wo(1024, inf["sun_dir_local"], math.acos(inf["cos_cutoff"]), seed=91, scale=0.98).astype(np.float64)
    wo = np.concatenate([ref["sky"]["wo"], disc, _horizon_wo(1024, 92)])
    n = wo.shape[0]
    rng = np.random.default_rng(93)
    k = 4 if variant == "spectral" else 3
    lam = rng.uniform(330, 710, (4, n)).astype(np.float32)
    cot = rng.standard_normal((k, n)).astype(np.float32)
    d_wi = rng.standard_normal((n, 3)).astype(np.float32)
    si = _si(_world(ref["m"], wo), _lam(variant, lam))
    val, dval = em.eval_jvp_dir(si, _gpu(d_wi))
    grad = _np64(em.eval_vjp_dir(si, torch.from_numpy(cot).cuda()))
    dval = _np64(dval)
    assert np.isfinite(dval).all() and np.isfinite(grad).all()
    fwd, rev = cot.astype(np.float64) * dval, grad * d_wi.T.astype(np.float64)
    mag = np.abs(fwd).sum(axis=0) + np.abs(rev).sum(axis=0)
    ratio = np.abs(fwd.sum(axis=0) - rev.sum(axis=0)) / (1e-4 * mag + 1e-12)
    below = wo[:, 2] < 0
    assert below.sum() >= 100 and not dval[:, below].any() and not grad[:, below].any() and not _np64(val)[:, below].any()
    assert (mag[wo[:, 2] > 1e-4] > 0).all()
    print(f"{config} {variant}: adjointness, worst {ratio.max():.3e} of the 1e-4 bar (lane {int(ratio.argmax())} of {n})")
    assert (ratio <= 1.0).all(), (config, variant, float(ratio.max()))


# ---------------------------------------------------------------- 5. value
@pytest.mark.parametrize("variant", VARIANTS)
def test_jvp_dir_value_matches_the_oracle(variant):
    """jvp_dir's `out` is the reference-order eval: held to the oracles as eval_jvp's value is
    (tests/test_eval_jvp.py), not to eval_jvp's bits."""
    d = scene()
    em = ss.load_dict(d, variant=variant)
    o32, o64 = O.Oracle(d, variant, "jit", "f32"), O.Oracle(d, variant, "jit", "f64")
    wo = rays(o32)
    lam = np.random.default_rng(3).uniform(330, 710, (4, wo.shape[0])).astype(np.float32)
    lam_o = lam if variant == "spectral" else None
    val, _ = em.eval_jvp_dir(_si(_gpu(-wo), _lam(variant, lam)), _gpu(np.ones_like(wo)))
    ref32, ref64 = o32.eval(-wo, lam_o), o64.eval(-wo, lam_o)
    ref32, ref64 = (ref32.T, ref64.T) if variant == "spectral" else (ref32, ref64)
    inf = o32.info()
    sun = (wo @ inf["sun_dir_local"] >= inf["cos_cutoff"]) & (wo[:, 2] >= 0)
    assert sun.sum() >= 512
    assert_parity(val.cpu().numpy().T, ref32, ref64, sun, precision="reference")


# ---------------------------------------------------------------- 6. launch shapes
@functools.lru_cache(maxsize=None)
def _small(variant):
    """N_SMALL rays: a hemisphere with every fourth lane inside the sun disc (disc lanes in the
    shortest prefixes too), 16 wavelength planes, a tangent and a 16-plane cotangent."""
    d = scene()
    em = ss.load_dict(d, variant=variant)
    inf = O.Oracle(d, variant, "jit", "f32").info()
    wo = hemisphere_wo(N_SMALL, seed=31)
    wo[::4] = sun_cone_wo(len(wo[::4]), inf["sun_dir_local"], np.arccos(inf["cos_cutoff"]), seed=32, scale=0.9)
    rng = np.random.default_rng(33)
    lam = rng.uniform(330, 710, (16, N_SMALL)).astype(np.float32)
    k = 16 if variant == "spectral" else 3
    return dict(em=em, wi=_gpu(-wo), d_wi=_gpu(rng.standard_normal((N_SMALL, 3))),
                cot=torch.from_numpy(rng.standard_normal((k, N_SMALL)).astype(np.float32)).cuda(),
                lam=torch.from_numpy(lam).cuda() if variant == "spectral" else None)


def _planes(s, variant, nlam=4):
    """(lam, cot) with nlam planes for the spectral variant, (None, 3-plane cot) for RGB."""
    if variant != "spectral":
        return None, s["cot"]
    return s["lam"][:nlam].contiguous(), s["cot"][:nlam].contiguous()


@pytest.mark.parametrize("variant", VARIANTS)
def test_prefixes_give_the_bits_of_the_full_batch(variant):
    s = _small(variant)
    em = s["em"]
    lam, cot = _planes(s, variant)
    full_v, full_d = em.eval_jvp_dir(_si(s["wi"], lam), s["d_wi"])
    full_g = em.eval_vjp_dir(_si(s["wi"], lam), cot)
    for k in PREFIXES:
        si = _si(_head(s["wi"], k), _head(lam, k))
        v, dv = em.eval_jvp_dir(si, _head(s["d_wi"], k))
        g = em.eval_vjp_dir(si, _head(cot, k))
        assert v.shape == dv.shape == (full_v.shape[0], k) and g.shape == (3, k)
        assert _same_bits(v, full_v[:, :k]) and _same_bits(dv, full_d[:, :k]), k
        assert _same_bits(g, full_g[:, :k]), k
    torch.cuda.synchronize()


@pytest.mark.parametrize("nlam", [1, 3, 4, 16])
def test_spectral_plane_counts(nlam):
    """Forward: plane q of an nlam-plane call has the bits of the single-plane call on q's
    wavelengths.  Reverse: with the cotangent on plane q only, the nlam-plane gradient equals
    the single-plane call's (the other planes add zeros)."""
    s = _small("spectral")
    em = s["em"]
    lam, cot = _planes(s, "spectral", nlam)
    val, dval = em.eval_jvp_dir(_si(s["wi"], lam), s["d_wi"])
    assert val.shape == dval.shape == (nlam, N_SMALL)
    assert em.eval_vjp_dir(_si(s["wi"], lam), cot).shape == (3, N_SMALL)
    for q in range(nlam):
        one = _si(s["wi"], lam[q:q + 1].contiguous())
        v1, d1 = em.eval_jvp_dir(one, s["d_wi"])
        assert _same_bits(val[q], v1[0]) and _same_bits(dval[q], d1[0]), (nlam, q)
        hot = torch.zeros_like(cot)
        hot[q] = cot[q]
        assert torch.equal(em.eval_vjp_dir(_si(s["wi"], lam), hot), em.eval_vjp_dir(one, cot[q:q + 1].contiguous())), (nlam, q)


@pytest.mark.parametrize("variant", VARIANTS)
def test_small_call_after_a_large_one_and_overwritten_gradient(variant):
    s = _small(variant)
    em = s["em"]
    lam, cot = _planes(s, variant)
    reps = 64   # 262k rays: more than one workgroup per CU
    big = lambda x: None if x is None else x.repeat(1, reps)   # noqa: E731
    ref_g = em.eval_vjp_dir(_si(s["wi"], lam), cot)
    ref_v, ref_d = em.eval_jvp_dir(_si(s["wi"], lam), s["d_wi"])
    bv, bd = em.eval_jvp_dir(_si(big(s["wi"]), big(lam)), big(s["d_wi"]))
    bg = em.eval_vjp_dir(_si(big(s["wi"]), big(lam)), big(cot))
    for r in (0, reps - 1):
        sl = slice(r * N_SMALL, (r + 1) * N_SMALL)
        assert _same_bits(bv[:, sl], ref_v) and _same_bits(bd[:, sl], ref_d) and _same_bits(bg[:, sl], ref_g)
    si = _si(_head(s["wi"], 65), _head(lam, 65))
    v, dv = em.eval_jvp_dir(si, _head(s["d_wi"], 65))
    assert _same_bits(v, ref_v[:, :65]) and _same_bits(dv, ref_d[:, :65])
    # the gradient is written, not accumulated: a poisoned output buffer is overwritten
    out = torch.full((3, 65), float("nan"), device="cuda")
    g = em.eval_vjp_dir(si, _head(cot, 65), out=out)
    assert g is out and _same_bits(out, ref_g[:, :65])
    out.fill_(1e30)
    em.eval_vjp_dir(si, _head(cot, 65), out=out)
    assert _same_bits(out, ref_g[:, :65])


# ---------------------------------------------------------------- 7. mask and edges
@pytest.mark.parametrize("variant", VARIANTS)
def test_mask(variant):
    """Masked lanes, with NaN directions, tangents, cotangents and wavelengths, give exactly 0 in
    every output; the others give the bits of the unmasked call on clean inputs."""
    s = _small(variant)
    em = s["em"]
    lam, cot = _planes(s, variant)
    on = torch.from_numpy(np.random.default_rng(34).random(N_SMALL) < 0.5).cuda()
    poison = lambda x: None if x is None else torch.where(on, x, torch.full_like(x, float("nan")))   # noqa: E731
    clean = (*em.eval_jvp_dir(_si(s["wi"], lam), s["d_wi"]), em.eval_vjp_dir(_si(s["wi"], lam), cot))
    si_p = _si(poison(s["wi"]), poison(lam))
    got = (*em.eval_jvp_dir(si_p, poison(s["d_wi"]), active=on), em.eval_vjp_dir(si_p, poison(cot), active=on))
    for name, a, b in zip(("val", "dval", "grad"), got, clean):
        assert bool((a[:, ~on] == 0).all()), f"{name}: a masked lane is not 0"
        assert _same_bits(a[:, on], b[:, on]), f"{name}: an unmasked lane differs"
    for off in (torch.zeros(N_SMALL, dtype=torch.bool, device="cuda"), False):
        outs = (*em.eval_jvp_dir(si_p, poison(s["d_wi"]), active=off), em.eval_vjp_dir(si_p, poison(cot), active=off))
        for a in outs:
            assert bool((a == 0).all()), off


@pytest.mark.parametrize("variant", VARIANTS)
def test_below_horizon_lanes_are_zero(variant):
    s = _small(variant)
    em = s["em"]
    lam, cot = _planes(s, variant)
    wi = s["wi"].clone()
    wi[2] = wi[2].abs()          # wo.z = -wi.z < 0 (or -0 where it was 0)
    wi[2].clamp_(min=1e-6)
    outs = (*em.eval_jvp_dir(_si(wi, lam), s["d_wi"]), em.eval_vjp_dir(_si(wi, lam), cot))
    for a in outs:
        assert bool((a == 0).all())


def test_invalid_wavelengths_are_zero():
    """Out-of-range and NaN wavelengths: exact zeros in the value, the tangent and the gradient;
    an invalid plane, even with a NaN cotangent, adds nothing to the gradient."""
    s = _small("spectral")
    em = s["em"]
    lam, cot = _planes(s, "spectral", 3)
    bad = torch.from_numpy(OUT_OF_RANGE[np.arange(N_SMALL) % len(OUT_OF_RANGE)]).cuda()[None]
    lam4 = torch.cat([lam[:2], bad, lam[2:]])
    cot4 = torch.cat([cot[:2], torch.full_like(bad, float("nan")), cot[2:]])
    val, dval = em.eval_jvp_dir(_si(s["wi"], lam4), s["d_wi"])
    assert bool((val[2] == 0).all()) and bool((dval[2] == 0).all())
    v3, d3 = em.eval_jvp_dir(_si(s["wi"], lam), s["d_wi"])
    assert _same_bits(val[[0, 1, 3]], v3) and _same_bits(dval[[0, 1, 3]], d3)
    assert _same_bits(em.eval_vjp_dir(_si(s["wi"], lam4), cot4), em.eval_vjp_dir(_si(s["wi"], lam), cot))
    g = em.eval_vjp_dir(_si(s["wi"], bad.repeat(4, 1)), torch.full((4, N_SMALL), float("nan"), device="cuda"))
    assert bool((g == 0).all())


@pytest.mark.parametrize("variant", VARIANTS)
def test_edge_directions_give_finite_results(variant):
    """cos theta == 0; wo equal to the sun direction; lanes on the limb; and, with the sun at
    the zenith, wi = (0, 0, -1)."""
    rng = np.random.default_rng(35)
    for sun in (None, [0.0, 0.0, 1.0]):
        d = scene(sun=sun)
        em = ss.load_dict(d, variant=variant)
        inf = O.Oracle(d, variant, "jit", "f32").info()
        s = np.asarray(inf["sun_dir_local"], np.float32)
        ph = rng.uniform(0, 2 * np.pi, 64)
        flat = np.stack([np.cos(ph), np.sin(ph), np.zeros(64)], 1)
        limb = sun_cone_wo(256, s, math.acos(inf["cos_cutoff"]), seed=36, scale=1.0)
        limb /= np.linalg.norm(limb, axis=1, keepdims=True)
        g = math.acos(inf["cos_cutoff"]) * (1 - np.array([1e-7, 1e-6, 1e-5, 1e-4, 1e-3]))[:, None]
        e1, _ = R.tangent_frame(s[None].astype(np.float64))
        rim = np.cos(g) * s + np.sin(g) * e1
        wo = np.concatenate([flat, s[None], [[0.0, 0.0, 1.0]], limb, rim]).astype(np.float32)
        n = wo.shape[0]
        k = 4 if variant == "spectral" else 3
        lam = _lam(variant, rng.uniform(330, 710, (4, n)).astype(np.float32))
        wi = _gpu(-wo)
        wi[2, :64] = 0.0   # +0 and -0
        wi[2, :32] = -0.0
        si = _si(wi, lam)
        val, dval = em.eval_jvp_dir(si, _gpu(rng.standard_normal((n, 3))))
        grad = em.eval_vjp_dir(si, torch.from_numpy(rng.standard_normal((k, n)).astype(np.float32)).cuda())
        for name, a in (("val", val), ("dval", dval), ("grad", grad)):
            assert bool(torch.isfinite(a).all()), (variant, sun, name, torch.nonzero(~torch.isfinite(a)).tolist()[:8])
        assert bool((val[:, :64] > 0).all()) and bool((val[:, 64] > val[:, 0]).all())   # horizon lanes active; the sun lane lit


# ---------------------------------------------------------------- 8. grid stride
def test_outputs_do_not_depend_on_the_grid(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 takes about 2.5 grid-stride steps per lane;
    this process makes the same calls at the default grid.  All four kernels, bit for bit."""
    n = W.batch_size()
    env = dict(os.environ, SUNSKY_AMD_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, W.__file__, str(n), str(tmp_path)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    inp = W.inputs(n)
    for variant in W.VARIANTS:
        with np.load(tmp_path / f"{variant}.npz") as stepped:
            single = W.run(variant, inp)
            assert sorted(stepped.files) == sorted(single)
            for name, a in single.items():
                b = stepped[name]
                assert a.shape == b.shape and a.shape[1] == n, (variant, name, a.shape, b.shape)
                same = (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))
                assert bool(same.all()), f"{variant} {name}: {int((~same).sum())} of {same.size} values differ"
                assert np.abs(a).max() > 0


# ---------------------------------------------------------------- 9. graph capture
@pytest.mark.parametrize("variant", VARIANTS)
def test_graph_capture_and_replay_after_a_parameter_update(variant):
    """Both calls are capturable (one stream, a single branch); a replay after
    parameters_changed_async with a new turbidity equals a direct call at the new state."""
    em = ss.SunskyEmitter(R.SCENES["mid"], variant)
    s = _small(variant)
    lam, cot = _planes(s, variant)
    si = _si(s["wi"], lam)

    def step():
        v, dv = em.eval_jvp_dir(si, s["d_wi"])
        return v, dv, em.eval_vjp_dir(si, cot)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step()
    g.replay()
    torch.cuda.synchronize()
    before = [c.clone() for c in captured]
    for a, b in zip(before, step()):
        assert _same_bits(a, b)
    params = em.traverse()
    params["turbidity"] = 6.5
    params.update()
    g.replay()
    torch.cuda.synchronize()
    eager = step()
    torch.cuda.synchronize()
    for a, b, old in zip(captured, eager, before):
        assert _same_bits(a, b)
        assert not torch.equal(a, old)


# ---------------------------------------------------------------- 10. autograd
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", ["fast", "reference"])
def test_eval_wi_forward_and_backward_bits(variant, precision):
    s = _small(variant)
    em = ss.SunskyEmitter(scene(), variant, precision=precision)
    lam, cot = _planes(s, variant)
    on = torch.from_numpy(np.random.default_rng(37).random(N_SMALL) < 0.8).cuda()
    for active in (None, on):
        wi = s["wi"].clone().requires_grad_(True)
        out = ss.eval_wi(em, wi, lam, active)
        assert _same_bits(out.detach(), em.eval(_si(s["wi"], lam), active))
        out.mul(cot).sum().backward()
        assert _same_bits(wi.grad, em.eval_vjp_dir(_si(s["wi"], lam), cot, active))
        assert float(wi.grad.abs().max()) > 0
    wi = s["wi"].clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(ss.eval_wi(em, wi, lam).sum(), wi, create_graph=True)
    with pytest.raises(RuntimeError):              # once_differentiable: no second derivatives
        g1.sum().backward()


@pytest.mark.parametrize("variant", VARIANTS)
def test_eval_wi_end_to_end_yaw_gradient(variant):
    """wi = -R(yaw) d0 with yaw a torch scalar leaf: d loss / d yaw of a fixed linear loss through
    torch's rotation and eval_wi, against a 4-point difference of the fp64 oracle over yaw
    (h = 2e-3), to 1e-3 of the contraction's magnitude (test_vjp_against_oracle_finite_differences'
    bar)."""
    d = R.SCENES["mid"]
    sun = np.asarray(O.Oracle(d, variant, "jit", "f32").info()["sun_dir_local"], np.float64)
    d0 = hemisphere_wo(4600, seed=41).astype(np.float64)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    yaw0, h = 0.3, 2e-3

    def rot(a):
        return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])

    # sky lanes over the whole stencil: yaw moves a direction by at most |d yaw|
    keep = (d0[:, 2] > 0.02) & (np.arccos(np.clip((d0 @ rot(yaw0).T) @ sun, -1, 1)) > 0.1 + 2 * h)
    d0 = d0[keep][:N_SMALL]
    n = d0.shape[0]
    assert n == N_SMALL
    rng = np.random.default_rng(42)
    k = 4 if variant == "spectral" else 3
    lam = rng.uniform(330, 710, (4, n)).astype(np.float32)
    w = rng.standard_normal((k, n)).astype(np.float32)
    o64 = O.Oracle(d, variant, "jit", "f64")

    def lanes(a):   # per-lane loss terms (n,) at yaw a
        v = o64.eval((-(d0 @ rot(a).T)).astype(np.float32), lam if variant == "spectral" else None)
        v = v if variant == "spectral" else v.T
        return (w.astype(np.float64) * v).sum(axis=0)

    with R.few_threads():
        c, c2 = R.d4(lambda s: lanes(yaw0 + s), h), R.d4(lambda s: lanes(yaw0 + s), h / 2)
    ref, mag = c.sum(), np.abs(c).sum()
    self_r = abs(c2.sum() - ref) / (1e-3 * mag)
    print(f"{variant}: oracle stencil over yaw, h vs h/2: {self_r:.3f} of the bar")
    assert self_r <= 0.1
    em = ss.load_dict(d, variant=variant)
    yaw = torch.tensor(yaw0, dtype=torch.float64, device="cuda", requires_grad=True)
    d0_t = torch.from_numpy(d0.T.copy()).cuda()
    cs, sn = torch.cos(yaw), torch.sin(yaw)
    wi = -torch.stack([cs * d0_t[0] - sn * d0_t[1], sn * d0_t[0] + cs * d0_t[1], d0_t[2]]).float()
    loss = (ss.eval_wi(em, wi, _lam(variant, lam)).double() * torch.from_numpy(w).cuda().double()).sum()
    loss.backward()
    got = float(yaw.grad)
    print(f"{variant}: d loss / d yaw {got:.6e}, oracle FD {ref:.6e}, {abs(got - ref) / (1e-3 * mag):.3f} of the 1e-3 bar")
    assert abs(got - ref) <= 1e-3 * mag, (got, ref, mag)
