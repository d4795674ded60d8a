"""CPU side of tests/test_gpu_direct_shapes.py: the oracle references its tests share, the bounds
they hold the kernels to (those of test_direct_diffuse.py / test_direct_conductor.py, restated as
functions so that one statement serves the fp32-against-fp64 check here and the GPU-against-fp32
check there), and self-checks of both.

The degenerate scenes (gpu_direct_worker.scene): sky only, sun only, the sun 95 degrees from the
zenith.  Before a kernel is held to the oracle on them, the oracle itself is checked here: every
value finite on all four scenes with the six axis normals among the 4096, the black scene exactly
zero, and the fp32 oracle inside the parity bounds against fp64 on the same inputs: the whole
estimators against the fp64 oracle on the fp32 oracle's own emitter samples, everything else
against the plain fp64 oracle (test_oracle_on_degenerate_scenes)."""
import functools

import numpy as np
import pytest

import oracle as O
import gpu_direct_worker as W
from test_direct_conductor import GOLD, Q, TOL, _gpu_views
from test_direct_diffuse import _gpu_normals, _rot_x

DEG_N, DEG_SPP, DEG_SEED = 4096, 2, 19
DEG_CONDUCTORS = W.CONDUCTORS[:2]         # Beckmann isotropic, GGX anisotropic
DIFFUSE_BOUND = (0.995, 2e-4)             # test_direct_diffuse_parity
CONDUCTOR_BOUND = (Q, TOL)                # test_direct_conductor_parity
EM_RAYS_BOUND = (2e-6, 1e-4)              # p99.9, max: both rays of test_direct_diffuse_rays_parity, emitter rays of
BSDF_RAYS_BOUND = (5e-4, 5e-2)            # test_direct_conductor_rays_parity; its BSDF rays


@functools.lru_cache(maxsize=None)
def degenerate_inputs():
    return W.inputs(DEG_N, DEG_SPP, seed=61, axes=True)


def make_oracle(frame, name, variant, precision="f32", w_sky=None):
    o = O.Oracle(W.scene(frame, name), variant, "jit", precision)
    if w_sky is not None:
        o.override_w_sky(w_sky)
    return o


def reference(o, inp, seed, spp, nlam=4, conductors=W.CONDUCTORS, vis=True, diffuse=True):
    """gpu_direct_worker.run_direct from the oracle `o` -> {the same names: numpy}: lighting
    (C, n) fp64, rays (spp, n, 3) fp32, weights (C, spp, n) fp64."""
    nrm, wi = inp["nrm"].T, inp["wi"].T
    lam = inp["lam"][:nlam] if o.spectral else None
    v = inp["vis"][:spp] if vis is True else vis
    out = {}
    if diffuse:
        out["diffuse"] = O.direct_diffuse(o, nrm, seed, spp, lam, inp["rho"], vis=v)
        out["diffuse_rays_em"], out["diffuse_rays_bs"] = O.direct_diffuse_rays(o, nrm, seed, spp)
    for dist, alpha in conductors:
        key = f"conductor_{dist}_{'aniso' if np.ndim(alpha) else 'iso'}"
        out[key] = O.direct_conductor(o, nrm, wi, alpha, dist, GOLD["eta"], GOLD["k"], seed, spp, lam, vis=v)
        e, b, w = O.direct_conductor_rays(o, nrm, wi, alpha, dist, seed, spp, GOLD["eta"], GOLD["k"])
        out.update({key + "_raysw_em": e, key + "_raysw_bs": b, key + "_raysw_bw": w})
    return out


@functools.lru_cache(maxsize=None)
def degenerate_reference(frame, name, variant, precision="f32", w_sky=None):
    """The oracle's outputs on degenerate_inputs(); w_sky: the sampling weight it adopts (the
    product's staged one; None = its own)."""
    o = make_oracle(frame, name, variant, precision, w_sky)
    return reference(o, degenerate_inputs(), DEG_SEED, DEG_SPP, 3, DEG_CONDUCTORS)


def rays_np(t):
    """A rays tensor (3, spp, n) of the wrappers -> (spp, n, 3) numpy, the oracle's layout."""
    return t.permute(1, 2, 0).cpu().numpy()


def check_lighting(got, ref, bound, what):
    """The per-point bound of test_direct_diffuse_parity / test_direct_conductor_parity: finite,
    the `q` quantile of the per-point relative difference below `tol`, the means within
    max(tol, 1e-3); where the reference is black (all zero), exact zeros."""
    q, tol = bound
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref)), what
    if not ref.any():
        assert not got.any(), f"{what}: {np.count_nonzero(got)} non-zero values where the reference is black"
        return 0.0
    rel = (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3 * np.abs(ref).max())).max(axis=0)
    quant = float(np.quantile(rel, q))
    print(f"{what}: rel quantiles (0.5, 0.99, {q}, 1) {np.quantile(rel, [0.5, 0.99, q, 1.0])}")
    assert quant < tol, (what, np.quantile(rel, [0.5, 0.99, q, 1.0]))
    assert abs(got.mean() - ref.mean()) < max(tol, 1e-3) * abs(ref.mean()), (what, got.mean(), ref.mean())
    return quant


def check_rays(g, o, bound, what):
    """The bounds of test_direct_*_rays_parity on one ray set (spp, n, 3): finite, the same lanes
    zeroed but for < 1e-3 of them, the others' directions within (p99.9, max) and unit length."""
    p999, mx = bound
    assert g.shape == o.shape, (what, g.shape, o.shape)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(o)), what
    zg, zo = ~g.any(axis=2), ~o.any(axis=2)
    assert (zg != zo).mean() < 1e-3, (what, (zg != zo).mean())
    both = ~zg & ~zo
    if not both.any():
        return 0.0
    dlt = np.abs(g[both].astype(np.float64) - o[both]).max(axis=1)
    print(f"{what}: {int(both.sum())} rays, p99.9 {np.quantile(dlt, 0.999):.3e}, max {dlt.max():.3e}, "
          f"pattern mismatch {(zg != zo).mean():.2e}")
    assert np.quantile(dlt, 0.999) < p999 and dlt.max() < mx, (what, np.quantile(dlt, 0.999), dlt.max())
    assert np.allclose(np.linalg.norm(g[both].astype(np.float64), axis=1), 1.0, atol=1e-5), what
    return float(dlt.max())


def check_weights(w_g, b_g, w_o, what):
    """The BSDF weights F G1 (C, spp, n) of test_direct_conductor_rays_parity: zero exactly where
    the BSDF direction is, within [0, 1], p99.9 within 1e-3 of the oracle's."""
    w_g, w_o = np.asarray(w_g, np.float64), np.asarray(w_o, np.float64)
    assert np.all(np.isfinite(w_g)), what
    assert np.array_equal(w_g.any(axis=0), b_g.any(axis=2)), what
    assert np.all((w_g >= 0) & (w_g <= 1)), what
    both = w_g.any(axis=0) & w_o.any(axis=0)
    if both.any():
        wr = (np.abs(w_g - w_o) / np.maximum(w_o, 1e-6)).max(axis=0)[both]
        print(f"{what}: {int(both.sum())} weights, rel quantiles (0.5, 0.99, 0.999, 1) {np.quantile(wr, [0.5, 0.99, 0.999, 1.0])}")
        assert np.quantile(wr, 0.999) < 1e-3, (what, np.quantile(wr, [0.5, 0.99, 0.999, 1.0]))


def check_all(got, ref, what, lighting=True):
    """Every output of run_direct / reference (numpy, the oracle's layouts) at its bound."""
    for name, r in ref.items():
        w = f"{what} {name}"
        if name.endswith("_bw"):
            check_weights(got[name], got[name[:-3] + "_bs"], r, w)
        elif "rays" in name:
            diffuse_or_em = name.startswith("diffuse") or name.endswith("_em")
            check_rays(got[name], r, EM_RAYS_BOUND if diffuse_or_em else BSDF_RAYS_BOUND, w)
        elif lighting:
            check_lighting(got[name], r, DIFFUSE_BOUND if name == "diffuse" else CONDUCTOR_BOUND, w)


# ---------------------------------------------------------------- self-checks
def test_worker_inputs_are_those_of_the_parity_tests():
    """The worker's input generators are the parity tests' (restated there so that the child
    process needs neither pytest nor the oracle), its verdicts cover 0..3 on every sample, the
    axis normals are exact and the inputs are reproducible."""
    nrm = W.normals(1000, 7)
    assert np.array_equal(nrm, _gpu_normals(1000, 7))
    assert np.array_equal(W.views(nrm, 8), _gpu_views(nrm, 8))
    assert np.array_equal(W.rot_x(0.35), _rot_x(0.35)) and W.GOLD == GOLD
    a, b = W.inputs(300, 3, axes=True), W.inputs(300, 3, axes=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert a["vis"].shape == (3, 300) and all(set(np.unique(r)) == {0, 1, 2, 3} for r in a["vis"])
    assert np.array_equal(a["nrm"].T[:6], [[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]])
    assert np.allclose(np.linalg.norm(a["nrm"], axis=0), 1, atol=1e-6)
    assert ((a["nrm"] * a["wi"]).sum(0) <= 0).any()          # some views below the surface
    assert W.scene("rotated", "sun_only")["sky_scale"] == 0.0 and "to_world" not in W.scene()
    assert abs(W.scene(name="below_horizon")["sun_direction"][2] - np.cos(np.deg2rad(95.0))) < 1e-12


def test_bounds_reject_what_they_should():
    """check_lighting / check_rays fail on a difference on 1 % of the points, on a NaN, on a
    non-zero value where the reference is black and on a changed zero pattern; they pass on
    the reference itself."""
    rng = np.random.default_rng(0)
    ref = rng.uniform(0.5, 1.0, (3, 2000))
    check_lighting(ref.copy(), ref, DIFFUSE_BOUND, "same")
    bad = ref.copy()
    bad[0, :20] *= 1.001
    with pytest.raises(AssertionError):
        check_lighting(bad, ref, DIFFUSE_BOUND, "1 % of points off by 1e-3")
    bad = ref.copy()
    bad[1, 5] = np.nan
    with pytest.raises(AssertionError):
        check_lighting(bad, ref, DIFFUSE_BOUND, "nan")
    zero = np.zeros((3, 100))
    check_lighting(zero.copy(), zero, DIFFUSE_BOUND, "black")
    bad = zero.copy()
    bad[2, 7] = 1e-30
    with pytest.raises(AssertionError):
        check_lighting(bad, zero, DIFFUSE_BOUND, "black but for one value")
    d = rng.standard_normal((2, 3000, 3))
    d = (d / np.linalg.norm(d, axis=2, keepdims=True)).astype(np.float32)
    d[0, :300] = 0
    check_rays(d.copy(), d, EM_RAYS_BOUND, "same")
    bad = d.copy()
    bad[1, :10] = 0
    with pytest.raises(AssertionError):
        check_rays(bad, d, EM_RAYS_BOUND, "10 of 6000 rays zeroed")
    bad = d.copy()
    bad[1, 0] = -bad[1, 0]
    with pytest.raises(AssertionError):
        check_rays(bad, d, EM_RAYS_BOUND, "one ray reversed")


def zero_pattern_mismatch(g, o):
    """Share of the rays (spp, n, 3) that one side zeroes and the other does not."""
    return float((~g.any(axis=2) != ~o.any(axis=2)).mean())


class OnSamplesOf:
    """The fp64 oracle `o64` on the emitter samples of the fp32 oracle `o32`: sample_direction
    returns o32's direction and pdf (its fp32 values) with the weight o64.eval(-d) / pdf, and eval
    and pdf_direction are o64's.  Through direct_diffuse / direct_conductor this is the fp64 value
    of the estimator on the samples the fp32 sampler drew: radiance at the sampled direction,
    BSDF terms and MIS in fp64, the sampler's (d, pdf) taken as given (the sampling parity tests
    hold those)."""

    def __init__(self, o32, o64):
        self.o32, self.o64, self.spectral = o32, o64, o32.spectral

    def eval(self, wi, wavelengths=None):
        return self.o64.eval(wi, wavelengths) if self.spectral else self.o64.eval(wi)

    def pdf_direction(self, d):
        return self.o64.pdf_direction(d)

    def sample_direction(self, sample, wavelengths=None):
        r = self.o32.sample_direction(sample, wavelengths=wavelengths)
        d = r["d"].astype(np.float32)
        pdf = r["pdf"].astype(np.float64)
        e = self.o64.eval(-d, wavelengths).T if self.spectral else self.o64.eval(-d)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(pdf[:, None] > 0, e / pdf[:, None], 0.0)
        return {"d": d.astype(np.float64), "pdf": pdf, "weight": w}


def measure(a, b, what):
    """Print (never assert) how two outputs of reference() differ: lighting (C, n) by the parity
    tests' per-point metric, rays (spp, n, 3) by component."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.ndim == 2:
        if not b.any():
            print(f"{what}: black, {np.count_nonzero(a)} non-zero")
            return
        rel = (np.abs(a - b) / np.maximum(np.abs(b), 1e-3 * np.abs(b).max())).max(axis=0)
        print(f"{what}: rel quantiles (0.5, 0.99, 0.995, 1) {np.quantile(rel, [0.5, 0.99, 0.995, 1.0])}")
    else:
        both = a.any(axis=2) & b.any(axis=2)
        d = np.abs(a[both] - b[both]).max(axis=1)
        if d.size:
            print(f"{what}: {d.size} rays, p99.9 {np.quantile(d, 0.999):.3e}, max {d.max():.3e}")


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_on_samples_of_itself_is_the_oracle(variant):
    """OnSamplesOf(o, o) is o: the weight sample_direction returns is eval(-d) / pdf, so the
    construction changes nothing but the precision of what it is given (fp32 rounding of the
    quotient: 1e-6, far inside the bounds)."""
    o32 = make_oracle("rotated", "base", variant)
    inp = W.inputs(512, 2, seed=71)
    check_all(reference(OnSamplesOf(o32, o32), inp, 3, 2, 3, DEG_CONDUCTORS), reference(o32, inp, 3, 2, 3, DEG_CONDUCTORS),
              f"{variant} on its own samples")


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
@pytest.mark.parametrize("frame", W.FRAMES)
@pytest.mark.parametrize("name", W.SCENES)
def test_oracle_on_degenerate_scenes(name, frame, variant):
    """On each scene, with the six axis normals among the 4096 points, spp 2 and three
    wavelengths: all the oracle returns (direct_diffuse, direct_diffuse_rays, direct_conductor,
    direct_conductor_rays with weights) is finite; w_sky is 1 for sky only and 0 for sun only and
    for the black scene, whose lighting is exactly zero.

    The fp32 oracle alone is then held to fp64 at the parity bounds, every output:
      * the whole estimators (both halves, random verdicts) against the fp64 oracle on the fp32
        oracle's own emitter samples (OnSamplesOf);
      * the BSDF-sampled half (bit 0 of every verdict cleared), the BSDF rays and their weights
        and which rays are zeroed against the plain fp64 oracle (given the fp32 oracle's w_sky, as
        the fp32 oracle is given the product's in the GPU test: their own differ by 2e-3
        relative, which would move the sky / sun pick of that share of samples).
    Against the plain fp64 oracle the emitter-sampled half is outside the bounds on any scene
    with an emitter sample, whatever the normals, because the two draw different samples: the
    fp32 inversion of the sky mixture moves a direction by up to 1e-3, and an fp32 direction
    places a sample inside the 0.27 degree sun cone to ~1e-3 of its radius, which the
    limb-darkened radiance repeats (and the fp32 1 - cos(cutoff) of the cone's pdf is 2.2e-3 off).
    Those figures are printed, not asserted (profiles/direct_shapes_pytest_cpu.log)."""
    o32 = make_oracle(frame, name, variant)
    w = o32.info()["w_sky"]
    if name != "base":
        assert w == (1.0 if name == "sky_only" else 0.0)
    inp = degenerate_inputs()
    r32 = degenerate_reference(frame, name, variant)
    r64 = degenerate_reference(frame, name, variant, "f64", w)
    for k, v in r32.items():
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(r64[k])), (name, variant, k)
    lighting = [k for k in r32 if "rays" not in k]
    if name == "below_horizon":
        assert not any(r32[k].any() or r64[k].any() for k in lighting)
    else:
        assert all(v.any() for v in r32.values())
    what = f"{name} {frame} {variant} f32 vs f64"
    on32 = reference(OnSamplesOf(o32, make_oracle(frame, name, variant, "f64", w)), inp, DEG_SEED, DEG_SPP, 3,
                     DEG_CONDUCTORS)
    check_all(r32, on32, what + " on the fp32 samples")
    for k in r32:
        if k.endswith("_bs") or k.endswith("_bw"):
            check_all(r32, {k: r64[k]}, what)
        elif k.endswith("_em"):
            assert zero_pattern_mismatch(r32[k], r64[k]) < 1e-3, (what, k)
    # the BSDF-sampled half alone: the same calls with bit 0 of every verdict cleared
    half = [reference(make_oracle(frame, name, variant, p, w), inp, DEG_SEED, DEG_SPP, 3, DEG_CONDUCTORS,
                      vis=inp["vis"][:DEG_SPP] & 2) for p in ("f32", "f64")]
    check_all({k: half[0][k] for k in lighting}, {k: half[1][k] for k in lighting}, what + " BSDF half")
    for k in lighting + [k for k in r32 if k.endswith("_em")]:
        measure(r32[k], r64[k], f"{what}, its own samples (measured only) {k}")
