"""CPU side of tests/test_gpu_sampling_shapes.py: the restatements of sampling_shapes_reference.py
anchored to the oracle, the fp32 oracle's own figures on the bounds the GPU tests hold the
sample_ray kernels to, and self-checks of the input generators.

The origin bound: per component |o - ray_origin(d)| <= 2 K32 origin_unit, where K32 is the fp32
oracle's own worst ratio on the same samples against the same restatement at the oracle's own
directions (ray_figures).  The two frame-independent invariants (|q . d| and ||q| - |r||, q the
ray's offset on its disk) are held to twice the fp32 oracle's own worst value likewise.  The
factor 2 covers what a kernel may differ in from the fp32 reference and still be as accurate:
sincos_fast's 1.56 ulp / 9.3e-8 absolute (tests/test_gpu_device_math.py), one v_rcp ulp on phi, another libm."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import sampling_shapes_reference as S
from helpers import fp32_sun_input

RAY_N = 1 << 15
COMBOS = [(v, s, f, sc) for v in ("rgb", "spectral") for s in ("jit", "scalar") for f in ("identity", "rotated")
          for sc in ("small", "large")]
IDS = ["-".join(c) for c in COMBOS]
MARGIN = 2.0          # the kernels against the fp32 oracle's own figure
K32_CEILING = 8.0     # sanity only: an fp32 origin is under a dozen roundings of at most half a unit each


def scene_dict(d, scene):
    c, r = S.SCENES[scene] if isinstance(scene, str) else scene
    return dict(d, bsphere_center=tuple(float(x) for x in c), bsphere_radius=float(r))


def make_oracles(d, variant, semantics, scene, em=None):
    """(o32, o64) of emitter dict d in the scene (a name of S.SCENES or (centre, radius)); em: the
    product emitter whose staged sampling state (w_sky, wavelength nodes) both adopt."""
    sd = scene_dict(d, scene)
    o32 = O.Oracle(sd, variant, semantics, "f32")
    # the fp64 oracle on the fp32 sun direction the product and o32 use (helpers.fp32_sun_input)
    o64 = O.Oracle(fp32_sun_input(sd, o32), variant, semantics, "f64")
    if em is not None:
        o32.adopt_sampling_state(em)
        o64.adopt_sampling_state(em)
    return o32, o64


def ray_figures(o, d, s2, center, radius):
    """(origin ratio, max |q . d|, max ||q| - |r||) of origins o (n, 3) at directions d (n, 3)."""
    d32 = np.asarray(d, np.float32)
    return (S.origin_ratio(o, d32, s2, center, radius),) + S.origin_invariants(o, d32, s2, center, radius)


def assert_ray_bounds(fig, fig32, what):
    """fig: a candidate's ray_figures, fig32: the fp32 oracle's on the same samples."""
    print(f"ORIGIN | {what} | ratio {fig[0]:.3f} (2 K32 = {MARGIN * fig32[0]:.3f}) | q.d {fig[1]:.3e} "
          f"(bound {MARGIN * fig32[1]:.3e}) | |q|-|r| {fig[2]:.3e} (bound {MARGIN * fig32[2]:.3e})")
    assert fig[0] <= MARGIN * fig32[0], f"{what}: origin ratio {fig[0]:.3f} over 2 K32 = {MARGIN * fig32[0]:.3f}"
    assert fig[1] <= MARGIN * fig32[1], f"{what}: |q . d| {fig[1]:.3e} over {MARGIN * fig32[1]:.3e}"
    assert fig[2] <= MARGIN * fig32[2], f"{what}: ||q| - |r|| {fig[2]:.3e} over {MARGIN * fig32[2]:.3e}"


WRAP_BAND = 1e-6      # radians


def tgmm_azimuth(o32, d_world, to_world=None):
    """The azimuth the sky pdf's gaussians see (compute_pdfs, sunsky.cpp:711-723): atan2(l.y, l.x) -
    (sun_phi - pi / 2) wrapped into [0, 2 pi), l the direction in the emitter's frame; fp64."""
    d = np.asarray(d_world, np.float64)
    loc = d if to_world is None else d @ np.asarray(to_world, np.float64)[:3, :3]
    phi = np.arctan2(loc[:, 1], loc[:, 0]) - (float(o32.info()["sun_angles"][0]) - 0.5 * np.pi)
    return np.mod(phi, 2.0 * np.pi), loc


def pdf_reference(o32, d_world, gp, to_world=None):
    """o32.pdf_direction at d_world (n, 3) -> (pdf, wrap lanes).  The gaussians are not periodic, so
    the sky pdf jumps where the azimuth wraps from 2 pi to 0 (3.3 % at the test emitter), and a
    sample with u.x = 0 lands exactly there (the first gaussian's azimuth truncated at 0): which
    side an fp32 evaluation takes is decided by one rounding of its atan2.  On lanes within
    WRAP_BAND of the wrap the reference is therefore two-valued: the direction is turned by
    +-2 WRAP_BAND about the zenith and the side nearer to the candidate's pdf gp is taken
    (test_pdf_jumps_where_the_azimuth_wraps)."""
    d = np.asarray(d_world, np.float32)
    pref = o32.pdf_direction(d).astype(np.float64)
    phi, loc = tgmm_azimuth(o32, d, to_world)
    wrap = np.minimum(phi, 2.0 * np.pi - phi) < WRAP_BAND
    if wrap.any():
        m = np.eye(3) if to_world is None else np.asarray(to_world, np.float64)[:3, :3]
        sides = []
        for eps in (2 * WRAP_BAND, -2 * WRAP_BAND):
            c, s = np.cos(eps), np.sin(eps)
            t = loc[wrap] @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])
            sides.append(o32.pdf_direction((t @ m.T).astype(np.float32)).astype(np.float64))
        g = np.asarray(gp, np.float64)[wrap]
        pref[wrap] = np.where(np.abs(sides[0] - g) <= np.abs(sides[1] - g), sides[0], sides[1])
    return pref, wrap


@functools.lru_cache(maxsize=None)
def _oracle_rays(variant, semantics, frame, scene):
    d = S.emitter_dict(frame)
    o32, o64 = make_oracles(d, variant, semantics, scene)
    ws, s2, s3 = S.ray_inputs(RAY_N, o32.info()["w_sky"])
    return s2, o32.sample_ray(ws, s2, s3), o64.sample_ray(ws, s2, s3)


@pytest.mark.parametrize("variant,semantics,frame,scene", COMBOS, ids=IDS)
def test_restatement_reproduces_the_fp64_oracle(variant, semantics, frame, scene):
    """ray_origin() at the fp64 oracle's own directions against its origins: within 1e-6 of the
    unit 2^-24 (|c_i| + 2 R) on 32,768 samples with the disk's centre, corners and edge midpoints."""
    s2, _, r64 = _oracle_rays(variant, semantics, frame, scene)
    c, r = S.SCENES[scene]
    ratio = S.origin_ratio(r64["o"], r64["d"], s2, c, r)
    print(f"restatement against o64 {variant} {semantics} {frame} {scene}: {ratio:.3e} units")
    assert ratio <= 1e-6
    assert np.isfinite(r64["o"]).all() and np.abs(np.linalg.norm(r64["d"], axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("variant,semantics,frame,scene", COMBOS, ids=IDS)
def test_fp32_oracle_is_inside_the_ray_bounds(variant, semantics, frame, scene):
    """K32 and the two invariants of the fp32 oracle, printed; the fp32 oracle passes the bounds the
    kernels are held to (the reference is never what fails)."""
    s2, r32, r64 = _oracle_rays(variant, semantics, frame, scene)
    c, r = S.SCENES[scene]
    fig32 = ray_figures(r32["o"], r32["d"], s2, c, r)
    assert_ray_bounds(fig32, fig32, f"o32 {variant} {semantics} {frame} {scene}")
    assert 0 < fig32[0] <= K32_CEILING, fig32
    assert fig32[1] < 2e-6 and fig32[2] < 2e-6, fig32


def _digest(n, w):
    h = hashlib.sha256()
    for k, v in sorted(S.inputs(n, w).items()):
        h.update(k.encode() + np.ascontiguousarray(v).tobytes())
    for kind in S.MASKS[1:]:
        h.update(S.mask(kind, n).tobytes())
    return h.hexdigest()


def test_input_generators_are_deterministic():
    """Twice in this process and once in a child process: the same bytes."""
    a, b = _digest(4099, 0.43), _digest(4099, 0.43)
    assert a == b and a != _digest(4099, 0.44)
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_sampling_shapes_cpu as T; print(T._digest(4099, 0.43))"
            % (here, os.path.join(os.path.dirname(here), "oracle")))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[-1] == a, r.stdout[-2000:]


def test_inputs_hold_the_specials():
    w = 0.43
    inp = S.inputs(4099, w)
    sp = S.special_samples(w)
    assert np.array_equal(inp["u"][0, :5], sp) and sp[0] == np.float32(w) and sp[1] < sp[0] < sp[2]
    assert sp[3] == 0 and sp[4] == np.float32(1 - 2.0 ** -24)
    assert (inp["u"][0, S.SKY_ROWS] < np.float32(w)).all() and (inp["u"][0, S.SUN_ROWS] >= np.float32(w)).all()
    assert (inp["u"] >= 0).all() and (inp["u"] < 1).all() and (inp["s2"] >= 0).all() and (inp["s2"] < 1).all()
    for win in (256, 192):      # each stretch covers whole windows of both kinds
        for rows in (S.SKY_ROWS, S.SUN_ROWS):
            assert rows.start % win == 0 and rows.stop % win == 0
    assert np.array_equal(inp["s2"][:, :12].T, S.DISK_SPECIALS)
    assert np.array_equal(inp["lam"][3, 1100:1111], S.NODES) and np.array_equal(inp["lam"][0, 1200:1206], S.EDGE_LAMBDA)
    assert inp["lam"].shape == (S.MAX_LAMBDA, 4099)
    assert np.abs(np.linalg.norm(inp["wo"], axis=0) - 1).max() < 1e-6
    for w_edge in (0.0, 1.0):   # the one-sided mixtures: still inside [0, 1)
        u = S.inputs(4099, w_edge)["u"]
        assert (u >= 0).all() and (u < 1).all()


@pytest.mark.parametrize("n", S.SIZES + (64, 128, 4096))
def test_mixed_mask_differs_within_every_row_of_64(n):
    m = S.mask("mixed", n)
    assert m.shape == (n,) and m.dtype == bool
    for base in range(0, n, 64):
        row = m[base:base + 64]
        if row.size >= 2:
            assert row.any() and not row.all(), base
    assert S.mask("none", n) is None and S.mask("all_true", n).all() and not S.mask("all_false", n).any()


def test_disk_and_frame_restatements():
    """disk(): on the unit disk, |off| = |r|, the specials where they belong; frame(): (s, t, d)
    orthonormal for unit d, the -z axis included."""
    off, r = S.disk(S.DISK_SPECIALS)
    assert np.allclose(np.linalg.norm(off, axis=1), np.abs(r), atol=1e-15)
    assert np.array_equal(off[0], [0.0, 0.0]) and np.allclose(off[1], -np.sqrt(0.5) * np.ones(2))
    assert np.allclose(off[5], [0, -1]) and np.allclose(off[7], [-1, 0])
    rng = np.random.default_rng(1)
    d = rng.standard_normal((1000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:2] = [[0, 0, 1], [0, 0, -1]]
    s, t = S.frame(d)
    for a, b in ((s, t), (s, d), (t, d)):
        assert np.abs((a * b).sum(1)).max() < 1e-14
    assert np.allclose(np.cross(s, t), d, atol=1e-14)


@pytest.mark.parametrize("semantics", ["jit", "scalar"])
def test_oracle_sample_direction_takes_any_wavelength_count(semantics):
    """o32.sample_direction with 1, 3, 5, 8 and 16 wavelength rows: d and pdf are those of the 4-row
    call, and every weight row equals the row a 4-row call gives for the same wavelengths."""
    o32 = O.Oracle(S.emitter_dict("rotated"), "spectral", semantics, "f32")
    n = 2048
    inp = S.inputs(n, o32.info()["w_sky"])
    u, lam = inp["u"].T, inp["lam"]
    four = [o32.sample_direction(u, wavelengths=lam[4 * j:4 * j + 4]) for j in range(4)]
    for k in (1, 3, 5, 8, 16):
        got = o32.sample_direction(u, wavelengths=lam[:k])
        assert got["weight"].shape == (n, k)
        assert np.array_equal(got["d"], four[0]["d"]) and np.array_equal(got["pdf"], four[0]["pdf"])
        for row in range(k):
            assert np.array_equal(got["weight"][:, row], four[row // 4]["weight"][:, row % 4]), (k, row)
    assert np.isfinite(four[0]["weight"]).all() and (four[0]["weight"] > 0).any()


def test_header_documents_the_four_wavelength_planes_of_sample_ray():
    """sunsky_sample_ray stores four wavelength planes in RGB too (zeros): the C header says so, and
    test_gpu_sampling_shapes.py canaries four rows."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "sunsky_amd.h")).read().replace("*", " ").split())
    assert "ray.wavelengths (4 planes; zeros in RGB)" in text


def test_pdf_jumps_where_the_azimuth_wraps():
    """The sample u.x = 0 of S.inputs puts the rotated test emitter's own direction on the azimuth
    wrap, where the reference's pdf_direction jumps; pdf_reference() flags that lane and returns the
    side it is asked for; away from the wrap it is pdf_direction.  (At the identity emitter's sun the
    same sample ends 5.7e-4 rad before the wrap: nothing is flagged.)"""
    d = S.emitter_dict("rotated")
    o32 = O.Oracle(d, "rgb", "jit", "f32")
    inp = S.inputs(4099, o32.info()["w_sky"])
    assert inp["u"][0, 3] == 0
    r = o32.sample_direction(inp["u"].T)
    tw = d["to_world"]
    phi, loc = tgmm_azimuth(o32, r["d"], tw)
    assert min(phi[3], 2 * np.pi - phi[3]) < 1e-7
    sides = []
    for eps in (2e-6, -2e-6):
        c, s = np.cos(eps), np.sin(eps)
        sides.append(o32.pdf_direction(((loc[3:4] @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])) @ tw[:3, :3].T).astype(np.float32))[0])
    jump = abs(sides[0] - sides[1]) / sides[0]
    print(f"pdf either side of the wrap {sides[0]:.7e} / {sides[1]:.7e} ({100 * jump:.2f} %), sampled {r['pdf'][3]:.7e}")
    assert jump > 1e-3 and min(abs(r["pdf"][3] - x) / x for x in sides) < 1e-5
    for want in sides:
        gp = r["pdf"].astype(np.float64).copy()
        gp[3] = want
        pref, wrap = pdf_reference(o32, r["d"], gp, tw)
        assert wrap[3] and wrap.sum() <= 2 and abs(pref[3] - want) <= 1e-6 * want
        assert np.array_equal(pref[~wrap], o32.pdf_direction(r["d"]).astype(np.float64)[~wrap])
    o_id = O.Oracle(S.emitter_dict("identity"), "rgb", "jit", "f32")
    r = o_id.sample_direction(S.inputs(4099, o_id.info()["w_sky"])["u"].T)
    pref, wrap = pdf_reference(o_id, r["d"], r["pdf"])
    assert not wrap.any() and np.array_equal(pref, o_id.pdf_direction(r["d"]).astype(np.float64))
