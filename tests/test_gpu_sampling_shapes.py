"""The sampling entry points at every call shape, stride, wavelength count and edge:
sunsky_sample_direction (RGB: the LEAN, kSortPos and kSortFull windows, the unsorted general and the
unsorted LEAN kernel; spectral: lean4_sorted, pos_sorted, spec_lean and the general spec kernel),
sunsky_sample_ray (sorted RGB, unsorted RGB, spectral), sunsky_pdf_direction (v4, v1) and
sunsky_sample_wavelengths, both precisions, a rotated (axis permutation) and an identity to_world,
set_scene([-1, -2, -3], [3, 2, 1]).  The parity tests hold these kernels' arithmetic to the oracle
through the Python wrapper (packed planes, four wavelengths, all or none of the optional pointers);
here (tests/gpu_sampling_worker.py makes the calls, tests/sampling_shapes_reference.py the inputs):

  1. strides, alignment and canaries through the C ABI: every stride n + 5, every plane base off
     16-byte alignment, outputs canaried; columns [0, n) == the packed call, every other element
     keeps the canary -- n ending inside, at and just past a window of 4 x 64 and of 3 x 64.
  2. wavelength counts of the spectral sample_direction: nlam 1, 2, 3 == the rows of nlam 4; nlam 5,
     8, 16: rows 0..3 == nlam 4, every row against the GPU's own eval and against the oracle;
     nlam 0 and 17 are refused and write nothing.
  3. every subset of {it_p, ds_dist, ds_p}, unmasked and masked.
  4. masked lanes: zero weight, zero pdf_direction, everything finite, active lanes == the unmasked
     call, and what an inactive lane holds otherwise.
  5. sample_ray against the references: ray.d == -sample_direction.d, the weights tied to
     sample_direction's, origins inside 2 K32 units and the frame-independent invariants on every
     lane, weights at the parity bars, over the sweep emitters, both semantics and two scenes.
  6. capped grid == default grid, bit for bit (a child process with SUNSKY_AMD_BLOCKS_PER_CU=1).
  7. a batch is a prefix of a longer batch, for the call shapes of 1 the other tests leave out.

Bit-for-bit comparisons count two NaNs as equal and require that none appears; all samples are in
range.  The references and bounds are those of test_sampling_shapes_cpu.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpu_sampling_worker as W
import sampler_disc_reference as DR
import sampling_shapes_reference as S
import sunsky_amd as ss
import test_sampling_shapes_cpu as R
from helpers import assert_parity, lambda_pdf, mask_flip_lanes, max_rel
from test_gpu_direct_shapes import assert_same_bits
from test_gpu_parity import SAMPLING_SWEEP

pytestmark = pytest.mark.gpu

VP = pytest.mark.parametrize("variant,precision", W.COMBOS, ids=["-".join(c) for c in W.COMBOS])
FRAMES = ("rotated", "identity")
UNSORTED, SORTED_GENERAL = "SUNSKY_AMD_UNSORTED_SAMPLING", "SUNSKY_AMD_SORTED_GENERAL_SAMPLING"
# the three sample_direction call shapes: (mask kind, it_p, ds_dist, ds_p)
SHAPES = {"lean": ("none", False, False, False), "general": ("none", True, True, True),
          "masked": ("mixed", True, True, True)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def emitter(variant, precision, frame="rotated"):
    return W.emitter(variant, precision, frame)


@functools.lru_cache(maxsize=None)
def inputs(variant, precision, frame, n):
    return W.inputs(emitter(variant, precision, frame), n)


def envs(variant, monkeypatch):
    """The kernel-selection switches, one at a time: none, unsorted and (RGB) sorted-general."""
    for env in (None, UNSORTED) + ((SORTED_GENERAL,) if variant == "rgb" else ()):
        if env:
            monkeypatch.setenv(env, "1")
        yield env or "default"
        if env:
            monkeypatch.delenv(env)


def same(got, want, what, lost=None):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert_same_bits(got[k], want[k], f"{what} {k}")
    for k, v in (lost or {}).items():
        assert v == 0, f"{what} {k}: {v} elements outside columns [0, n) were written"


def direction(em, inp, shape, nlam=4, strided=False, mask=None):
    kind, it_p, dist, pos = SHAPES[shape]
    n = inp["u"].shape[1]
    return W.sample_direction(em, inp, nlam, S.mask(kind, n) if mask is None else mask, it_p, dist, pos, strided)


# ---------------------------------------------------------------- 1
@VP
def test_sample_direction_strides_alignment_and_canaries(variant, precision, monkeypatch):
    """LEAN, general and masked general, each under no switch, SUNSKY_AMD_UNSORTED_SAMPLING and (RGB)
    SUNSKY_AMD_SORTED_GENERAL_SAMPLING, spectral at nlam 4 and 3: the strided call's columns [0, n)
    equal the packed call's, and padding, guards and the unused weight row keep the canary."""
    for frame in FRAMES:
        em = emitter(variant, precision, frame)
        for n in S.SIZES:
            inp = inputs(variant, precision, frame, n)
            for env in envs(variant, monkeypatch):
                for nlam in ((4, 3) if variant == "spectral" else (4,)):
                    for shape in SHAPES:
                        packed, _ = direction(em, inp, shape, nlam)
                        strided, lost = direction(em, inp, shape, nlam, strided=True)
                        same(strided, packed, f"{frame} n={n} {env} nlam={nlam} {shape}", lost)


@VP
def test_packed_c_calls_are_the_wrapper_calls(variant, precision):
    """The packed calls of the worker are what the Python wrapper passes: the same bits."""
    em = emitter(variant, precision)
    n = 4099
    inp = inputs(variant, precision, "rotated", n)
    t = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    lam = t["lam"][:4].contiguous() if variant == "spectral" else None
    ds, w = em.sample_direction(ss.Interaction3f(wavelengths=lam), t["u"], positions=False)
    same(direction(em, inp, "lean")[0], {"d": ds.d, "pdf": ds.pdf[None], "w": w}, "LEAN")
    ds, w = em.sample_direction(ss.Interaction3f(p=t["p"], wavelengths=lam), t["u"])
    same(direction(em, inp, "general")[0], {"d": ds.d, "pdf": ds.pdf[None], "w": w, "dist": ds.dist[None], "p": ds.p},
         "general")
    ray, w = em.sample_ray(None, t["ws"] if variant == "spectral" else None, t["s2"], t["u"])
    same(W.sample_ray(em, inp)[0], {"o": ray.o, "d": ray.d, "lam": ray.wavelengths, "w": w}, "sample_ray")
    pdf = em.pdf_direction(ss.Interaction3f(), ss.DirectionSample3f(d=t["wo"]))
    same(W.pdf_direction(em, inp)[0], {"pdf": pdf[None]}, "pdf_direction")
    lam_o, w = em.sample_wavelengths(ss.SurfaceInteraction3f(wi=-t["wo"]), t["ws"] if variant == "spectral" else None)
    same(W.sample_wavelengths(em, inp)[0], {"lam": lam_o, "w": w}, "sample_wavelengths")


@VP
def test_sample_ray_strides_alignment_and_canaries(variant, precision, monkeypatch):
    """Unmasked (RGB: the wave-sorted windows, which compute lanes past the end of the batch),
    masked and unsorted.  ray.wavelengths has four canaried rows in RGB too: the kernels store four
    planes of zeros there (include/sunsky_amd.h)."""
    for frame in FRAMES:
        em = emitter(variant, precision, frame)
        for n in S.SIZES:
            inp = inputs(variant, precision, frame, n)
            for env in (None, UNSORTED):
                if env:
                    monkeypatch.setenv(env, "1")
                for kind in ("none", "mixed"):
                    packed, _ = W.sample_ray(em, inp, S.mask(kind, n))
                    strided, lost = W.sample_ray(em, inp, S.mask(kind, n), strided=True)
                    same(strided, packed, f"{frame} n={n} {env} mask={kind}", lost)
                    if variant == "rgb":
                        assert int(torch.count_nonzero(strided["lam"])) == 0
                if env:
                    monkeypatch.delenv(env)


@VP
def test_pdf_direction_strides_alignment_and_canaries(variant, precision):
    """16-byte aligned pitched planes (a 4-directions-per-lane body plus a one-per-lane tail) and
    planes off 16-byte alignment (one per lane throughout), without and with a mask, against the
    packed call."""
    for frame in FRAMES:
        em = emitter(variant, precision, frame)
        for n in S.SIZES:
            inp = inputs(variant, precision, frame, n)
            for kind in ("none", "mixed"):
                packed, _ = W.pdf_direction(em, inp, S.mask(kind, n))
                for layout in ("pitched", "misaligned"):
                    got, lost = W.pdf_direction(em, inp, S.mask(kind, n), layout)
                    same(got, packed, f"{frame} n={n} mask={kind} {layout}", lost)


@VP
def test_sample_wavelengths_strides_alignment_and_canaries(variant, precision):
    for frame in FRAMES:
        em = emitter(variant, precision, frame)
        for n in S.SIZES:
            inp = inputs(variant, precision, frame, n)
            for kind in ("none", "mixed"):
                packed, _ = W.sample_wavelengths(em, inp, S.mask(kind, n))
                strided, lost = W.sample_wavelengths(em, inp, S.mask(kind, n), strided=True)
                same(strided, packed, f"{frame} n={n} mask={kind}", lost)


def test_pitched_planes_count_a_write_into_their_padding():
    p = W.Pitched(2, 101)
    p.columns(1)[:] = 1.0
    assert p.untouched() == 0 and p.stride == 108
    p.body[0, 101] = 2.0
    p.body[1, 0] = 2.0
    p.buf[15] = 2.0
    p.buf[-1] = 2.0
    assert p.untouched() == 4


# ---------------------------------------------------------------- 2
NLAM_N = 4099


@functools.lru_cache(maxsize=None)
def nlam_setup(precision, frame):
    em = emitter("spectral", precision, frame)
    o32, o64t, o64 = DR.oracles(S.emitter_dict(frame), "spectral", em)
    disc = DR.LocalDisc(em, 0.5358, to_local=S.PERMUTE[:3, :3].T if frame == "rotated" else None)
    return em, o32, o64t, o64, disc


def gpu_eval(em, gd, lam):
    si = ss.SurfaceInteraction3f(wi=torch.from_numpy(np.ascontiguousarray(-gd.T)).cuda(),
                                 wavelengths=torch.from_numpy(np.ascontiguousarray(lam)).cuda())
    return em.eval(si).cpu().numpy().T.astype(np.float64)


def check_rows_against_eval_and_oracle(precision, frame, inp, got, nlam, what):
    """Every weight row: weight * pdf == the GPU's own eval(-d) within 1e-5 relative plus the disc
    bound of test_gpu_sampler_disc_literal.check, and d, pdf, weight against the oracle (adopted
    w_sky) at the bars of test_gpu_parity.test_sample_direction_and_pdf_parity."""
    em, o32, o64t, o64, disc = nlam_setup(precision, frame)
    u, lam = inp["u"].T, inp["lam"][:nlam]
    gd, gp = got["d"].cpu().numpy().T.copy(), got["pdf"].cpu().numpy()[0].astype(np.float64)
    gw = got["w"].cpu().numpy().T.astype(np.float64)
    assert np.isfinite(gw).all() and gw.shape == (u.shape[0], nlam)
    ref = o32.sample_direction(u, wavelengths=lam)
    dir_err = np.abs(gd - ref["d"]).max(axis=1)
    print(f"{what}: |dd| p99.9 {np.quantile(dir_err, 0.999):.2e} max {dir_err.max():.2e}")
    assert np.quantile(dir_err, 0.999) < 2e-6 and dir_err.max() < 1e-4, what
    info = o32.info()
    sun_w = info["sun_dir_world"]
    inside = (gd @ sun_w) >= info["cos_cutoff"]
    same_formula = (u[:, 0] < np.float32(em.sky_sampling_w)) | inside
    pref, wrap = R.pdf_reference(o32, gd, gp, S.PERMUTE if frame == "rotated" else None)
    print(f"{what}: {int(wrap.sum())} lanes on the azimuth wrap, pdf max rel {max_rel(gp[same_formula], pref[same_formula]):.2e}")
    assert wrap.sum() <= 2 and max_rel(gp[same_formula], pref[same_formula]) < 1e-5, what
    up = gd @ S.PERMUTE[:3, 2] >= 0 if frame == "rotated" else gd[:, 2] >= 0
    ok = up & (gp > 0)
    safe = np.where(gp > 0, gp, 1.0)[:, None]
    lanes = (np.asarray(gd, np.float64) @ sun_w) >= info["cos_cutoff"] - 1e-6          # helpers.disc_lanes, world frame
    for j in range(0, nlam, 4):
        rows = slice(j, min(j + 4, nlam))
        k = rows.stop - rows.start
        l4 = np.concatenate([lam[rows], np.repeat(lam[rows][-1:], 4 - k, axis=0)])   # LocalDisc takes four rows
        e32, e64, e64t = (o.eval(-gd, l4).T.astype(np.float64) for o in (o32, o64, o64t))
        w4 = np.concatenate([gw[:, rows], np.repeat(gw[:, rows][:, -1:], 4 - k, axis=1)], axis=1)
        assert_parity(w4, (e32 / safe).astype(np.float32), e64 / safe, lanes, rtol=1e-5, precision=precision)
        tm = disc.terms(gd, l4)
        flip = DR.disc_flip_lanes(e32, e64t) & ok
        if flip.any():
            tm = disc.terms(gd, l4, hit=tm.hit ^ flip)
        t = np.where(flip[:, None], tm.eval, e64t) / safe
        bound = disc.bound(tm, t, gp)
        ge = gpu_eval(em, gd, l4)
        mis = np.abs(w4 * gp[:, None] - ge) <= bound * gp[:, None] + 1e-5 * np.abs(ge)
        assert mis[ok].all(), f"{what} rows {j}..: w pdf off eval on {int((~mis[ok]).any(axis=1).sum())} lanes"
        assert (w4[~up] == 0).all()


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("precision", ["fast", "reference"])
def test_wavelength_counts(precision, frame):
    """LEAN, general and masked general.  nlam 1, 2, 3 (eval_spec_one over S.ld) == the same rows of
    nlam 4 (eval_spec4 over S.ldp), d and pdf identical; nlam 5, 8, 16: rows 0..3 == nlam 4, every
    row against eval and the oracle; nlam 16 at lstride n + 5 == the packed call."""
    em = emitter("spectral", precision, frame)
    inp = inputs("spectral", precision, frame, NLAM_N)
    mk = S.mask("mixed", NLAM_N)
    for shape in SHAPES:
        four, _ = direction(em, inp, shape, 4)
        for nlam in (1, 2, 3, 5, 8, 16):
            got, _ = direction(em, inp, shape, nlam)
            what = f"{precision} {frame} {shape} nlam={nlam}"
            k = min(nlam, 4)
            assert tuple(got["w"].shape) == (nlam, NLAM_N)
            same({**got, "w": got["w"][:k]}, {**four, "w": four["w"][:k]}, what)
            if nlam > 4 and shape != "masked":
                check_rows_against_eval_and_oracle(precision, frame, inp, got, nlam, what)
            if shape == "masked":
                assert int(torch.count_nonzero(got["w"][:, torch.from_numpy(~mk).cuda()])) == 0, what
                lean, _ = direction(em, inp, "lean", nlam)
                act = torch.from_numpy(mk).cuda()
                assert_same_bits(got["w"][:, act], lean["w"][:, act], what + " active lanes against LEAN")
        kind, it_p, dist, pos = SHAPES[shape]
        for nlam in (16, 3):
            packed, _ = direction(em, inp, shape, nlam)
            strided, lost = direction(em, inp, shape, nlam, strided=True)
            same(strided, packed, f"{precision} {frame} {shape} nlam={nlam} strided", lost)
            # wl_stride and weight_stride that differ: lstride n + 5 with everything else packed, and
            # packed wavelengths (lstride n) with every other plane at n + 5 and canaried
            args = (em, inp, nlam, S.mask(kind, NLAM_N), it_p, dist, pos)
            same(W.sample_direction(*args, lam_strided=True)[0], packed, f"{precision} {frame} {shape} nlam={nlam} lstride n + 5")
            strided, lost = W.sample_direction(*args, strided=True, lam_strided=False)
            same(strided, packed, f"{precision} {frame} {shape} nlam={nlam} lstride n, wstride n + 5", lost)


@pytest.mark.parametrize("precision", ["fast", "reference"])
def test_wavelength_counts_out_of_range_are_refused(precision):
    """nlam 0 and 17: SUNSKY_ERROR_INVALID_VALUE, and no output element is written."""
    em = emitter("spectral", precision)
    inp = inputs("spectral", precision, "rotated", 257)
    for nlam in (0, 17):
        for shape in SHAPES:
            kind, it_p, dist, pos = SHAPES[shape]
            _, lost = W.sample_direction(em, inp, nlam, S.mask(kind, 257), it_p, dist, pos, strided=True,
                                         expect=W.INVALID_VALUE)
            assert not any(lost.values()), (nlam, shape, lost)


# ---------------------------------------------------------------- 3
SUBSETS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]


@VP
def test_partial_pointer_sets(variant, precision):
    """All eight subsets of {it_p, ds_dist, ds_p}, unmasked and masked: d, pdf and weight are the
    LEAN call's (under a mask the inactive columns of weight are 0; their pdf is compared in
    test_masked_lanes), ds_dist and ds_p those of the call with everything requested and the same
    it_p (none: the origin)."""
    em = emitter(variant, precision)
    n = 4099
    inp = inputs(variant, precision, "rotated", n)
    lean, _ = W.sample_direction(em, inp)
    mk = S.mask("mixed", n)
    act = torch.from_numpy(mk).cuda()
    for mask in (None, mk):
        full = {it_p: W.sample_direction(em, inp, 4, mask, it_p, True, True)[0] for it_p in (False, True)}
        for it_p, dist, pos in SUBSETS:
            got, _ = W.sample_direction(em, inp, 4, mask, it_p, dist, pos)
            strided, lost = W.sample_direction(em, inp, 4, mask, it_p, dist, pos, strided=True)
            what = f"it_p={it_p} ds_dist={dist} ds_p={pos} masked={mask is not None}"
            same(strided, got, what + " strided", lost)
            assert sorted(got) == sorted(["d", "pdf", "w"] + ["dist"] * dist + ["p"] * pos)
            assert_same_bits(got["d"], lean["d"], what + " d")
            if mask is None:
                assert_same_bits(got["pdf"], lean["pdf"], what + " pdf")
                assert_same_bits(got["w"], lean["w"], what + " w")
            else:
                assert_same_bits(got["pdf"][:, act], lean["pdf"][:, act], what + " pdf")
                assert_same_bits(got["w"][:, act], lean["w"][:, act], what + " w")
                assert int(torch.count_nonzero(got["w"][:, ~act])) == 0, what
                assert_same_bits(got["pdf"], full[it_p]["pdf"], what + " pdf on every lane")
            for k in ("dist", "p"):
                if k in got:
                    assert_same_bits(got[k], full[it_p][k], f"{what} {k}")
    # ds.dist = 2 max(R, |it.p - c|) and ds.p = it.p + d ds.dist: with it_p null, from the origin
    c, r = em.info()["bsphere_center"], em.info()["bsphere_radius"]
    want = 2.0 * max(float(r), float(np.linalg.norm(c)))
    assert np.allclose(full[False]["dist"].cpu().numpy(), want, rtol=1e-6)
    assert np.allclose(full[False]["p"].cpu().numpy(), full[False]["d"].cpu().numpy() * want, rtol=1e-6, atol=1e-6)


@VP
def test_half_set_vectors_are_refused(variant, precision):
    em = emitter(variant, precision)
    inp = inputs(variant, precision, "rotated", 65)
    for half, it_p, pos in (("it_p", True, False), ("ds_p", False, True), ("it_p", True, True)):
        _, lost = W.sample_direction(em, inp, 4, None, it_p, False, pos, strided=True, expect=W.INVALID_VALUE, half=half)
        assert not any(lost.values()), (half, lost)


# ---------------------------------------------------------------- 4
def _inactive(t, mask):
    return t[:, torch.from_numpy(~mask).cuda()]


def _active(t, mask):
    return t[:, torch.from_numpy(mask).cuda()]


@VP
def test_masked_lanes(variant, precision, monkeypatch):
    """Every entry point and kernel variant under an all-false, an all-true and a mixed mask (both
    values inside every row of 64): inactive lanes carry weight == 0 and pdf_direction == 0 and
    finite d, pdf, o and wavelengths; active lanes the unmasked call's bits.  What the code leaves
    on an inactive lane beyond that: the direction, the origin and the
    wavelengths of the unmasked call, bit for bit (they do not depend on the mask), and as sampled
    pdf the mixture's sun term alone (compute_pdfs masks the sky term only, as the reference does)
    -- never above the unmasked pdf.  The kernel variants agree on all of it bit for bit."""
    for frame in FRAMES:
        em = emitter(variant, precision, frame)
        for n in (257, 4099):
            inp = inputs(variant, precision, frame, n)
            for nlam in ((4, 3) if variant == "spectral" else (4,)):
                free, _ = direction(em, inp, "general", nlam)
                for kind in S.MASKS[1:]:
                    mk = S.mask(kind, n)
                    per_env = []
                    for env in envs(variant, monkeypatch):
                        got, _ = direction(em, inp, "masked", nlam, mask=mk)
                        what = f"sample_direction {frame} n={n} nlam={nlam} {kind} {env}"
                        same({k: _active(v, mk) for k, v in got.items()}, {k: _active(v, mk) for k, v in free.items()}, what)
                        assert int(torch.count_nonzero(_inactive(got["w"], mk))) == 0, what
                        for k in ("d", "dist", "p"):
                            assert_same_bits(got[k], free[k], f"{what} {k} on every lane")
                        assert bool(torch.isfinite(got["pdf"]).all()) and bool((got["pdf"] <= free["pdf"]).all()), what
                        per_env.append(got)
                    for other in per_env[1:]:
                        same(other, per_env[0], f"sample_direction {frame} n={n} nlam={nlam} {kind}: kernel variants")
            free, _ = W.sample_ray(em, inp)
            for kind in S.MASKS[1:]:
                mk = S.mask(kind, n)
                got, _ = W.sample_ray(em, inp, mk)
                what = f"sample_ray {frame} n={n} {kind}"
                same({k: _active(v, mk) for k, v in got.items()}, {k: _active(v, mk) for k, v in free.items()}, what)
                assert int(torch.count_nonzero(_inactive(got["w"], mk))) == 0, what
                for k in ("o", "d", "lam"):
                    assert_same_bits(got[k], free[k], f"{what} {k} on every lane")
                monkeypatch.setenv(UNSORTED, "1")
                same(W.sample_ray(em, inp, mk)[0], got, what + " unsorted")
                monkeypatch.delenv(UNSORTED)
            for layout in ("packed", "pitched", "misaligned"):
                free, _ = W.pdf_direction(em, inp, None, layout)
                for kind in S.MASKS[1:]:
                    mk = S.mask(kind, n)
                    got, _ = W.pdf_direction(em, inp, mk, layout)
                    what = f"pdf_direction {frame} n={n} {kind} {layout}"
                    assert_same_bits(_active(got["pdf"], mk), _active(free["pdf"], mk), what)
                    assert int(torch.count_nonzero(_inactive(got["pdf"], mk))) == 0, what
            free, _ = W.sample_wavelengths(em, inp)
            for kind in S.MASKS[1:]:
                mk = S.mask(kind, n)
                got, _ = W.sample_wavelengths(em, inp, mk)
                what = f"sample_wavelengths {frame} n={n} {kind}"
                same({k: _active(v, mk) for k, v in got.items()}, {k: _active(v, mk) for k, v in free.items()}, what)
                assert int(torch.count_nonzero(_inactive(got["w"], mk))) == 0, what
                assert_same_bits(got["lam"], free["lam"], what + " wavelengths on every lane")


# ---------------------------------------------------------------- 5
RAY_N = 1 << 14
RAY_EMITTERS = [("sweep%d" % i, c) for i, c in enumerate(SAMPLING_SWEEP)] + [("rotated", None)]
RAY_CASES = pytest.mark.parametrize(
    "variant,precision,semantics,name,case,scene",
    [(v, p, sem, name, case, sc) for v in ("rgb", "spectral") for p in ("fast", "reference") for sem in ("jit", "scalar")
     for name, case in RAY_EMITTERS for sc in S.SCENES],
    ids=lambda x: x if isinstance(x, str) else "")
TIE_ULP = 2.0 ** -23       # the spacing of fp32 at 1


class RayCase:
    pass


@functools.lru_cache(maxsize=2)
def ray_case(variant, precision, semantics, name, scene):
    """The emitter, the oracles (adopted sampling state), 16,384 samples with the specials of
    S.inputs, the unmasked sample_ray outputs and the sample_direction outputs for u = sample3
    (spectral: at the ray's own wavelengths); shared by the two tests below, read-only."""
    c = RayCase()
    case = dict(RAY_EMITTERS)[name]
    c.d = S.emitter_dict("rotated") if case is None else S.sweep_dict(case)
    c.em = em = ss.SunskyEmitter(c.d, variant, semantics, precision=precision)
    W.set_sphere(em, *S.SCENES[scene])
    info = em.info()
    # c and R as the emitter reports them (set_scene enlarges the radius by a ray epsilon)
    c.center, c.radius = tuple(float(x) for x in info["bsphere_center"]), float(info["bsphere_radius"])
    assert c.center == S.SCENES[scene][0] and 0 <= c.radius / S.SCENES[scene][1] - 1 < 1e-3
    c.o32, c.o64 = R.make_oracles(c.d, variant, semantics, (c.center, c.radius), em)
    c.w_sky = np.float32(em.sky_sampling_w)
    c.inp = inp = S.inputs(RAY_N, c.w_sky, seed=83)
    c.ws, c.s2, c.s3 = inp["ws"], inp["s2"].T, inp["u"].T
    got, _ = W.sample_ray(em, inp)
    c.ro, c.rd, c.lam, c.gw = (got[k].cpu().numpy().T.copy() for k in ("o", "d", "lam", "w"))
    ds, _ = W.sample_direction(em, {**inp, "lam": c.lam.T.copy()} if variant == "spectral" else inp)
    c.gd, c.gp, c.wd = ds["d"].cpu().numpy().T, ds["pdf"].cpu().numpy()[0].astype(np.float64), ds["w"].cpu().numpy().T
    return c


@RAY_CASES
def test_sample_ray_is_tied_to_sample_direction(variant, precision, semantics, name, case, scene):
    """Every lane, sky picks included: ray.d == -sample_direction(u = sample3).d, and pdf_ray ==
    ds.pdf c with c the reference's fp32 constant InvPi (1 / (R R)) (sunsky.cpp:354-397), checked
    on the weights: w_ray c == w_dir, where w_dir is sample_direction's weight (spectral: the
    GPU's own sample_wavelengths weight at the ray, eval / wavelength pdf, over ds.pdf).  Five
    correctly rounded fp32 operations separate the two sides (the product ds.pdf c, two
    reciprocals -- v_rcp's 1 ulp in the fast kernels -- and two products), so their distance in
    units in the last place of the weight reaches 3 for correct arithmetic; the bound of 2 ulp is
    held as 2 x 2^-23 relative (the fp32 spacing at 1).  Printed too: the distance in units in the
    last place against w_dir pi R^2 with pi R^2 exact (3 to 5; c alone is 0.8 / 1.3 x 2^-24 off
    1 / (pi R^2) in the two scenes).  Measured worst over the 36 cases of a kind: 1.98 x 2^-23 RGB
    fast (a thin margin: seven half-ulps are possible there), 1.27 RGB reference, 1.38 / 0.98
    spectral."""
    c = ray_case(variant, precision, semantics, name, scene)
    what = f"{variant} {precision} {semantics} {name} {scene}"
    assert np.isfinite(c.rd).all() and np.isfinite(c.gw).all(), what
    assert np.array_equal(c.rd, -c.gd), f"{what}: ray.d != -ds.d on {int((c.rd != -c.gd).any(axis=1).sum())} lanes"
    if variant == "spectral":
        wl, _ = W.sample_wavelengths(c.em, {"wo": -c.rd.T.copy(), "ws": c.ws})      # si.wi = the ray direction
        assert np.array_equal(wl["lam"].cpu().numpy().T, c.lam), what
        wdir = np.where((c.gp > 0)[:, None], wl["w"].cpu().numpy().T.astype(np.float64) / np.where(c.gp > 0, c.gp, 1.0)[:, None], 0.0)
    else:
        wdir = c.wd.astype(np.float64)
    r32 = np.float32(c.radius)
    c32 = float(np.float32(0.31830988618379067154) * (np.float32(1) / (r32 * r32)))
    tied = wdir / c32
    zero = tied == 0
    assert (c.gw[zero] == 0).all() and (c.gw[~zero] != 0).all(), f"{what}: the zero weights differ"
    rel = np.abs(c.gw[~zero] - tied[~zero]) / np.abs(tied[~zero])
    with np.errstate(over="ignore"):
        exact = (wdir * np.pi * c.radius ** 2).astype(np.float32)
    fin = np.isfinite(exact)
    print(f"RAYTIE | {what} | w_ray c against w_dir: {rel.max() / TIE_ULP:.2f} x 2^-23; w_ray against w_dir pi R^2: "
          f"{S.ulps(c.gw[fin], exact[fin])} ulp")
    assert rel.max() <= 2 * TIE_ULP, f"{what}: w_ray c is {rel.max() / TIE_ULP:.2f} x 2^-23 off w_dir"


@RAY_CASES
def test_sample_ray_against_the_references(variant, precision, semantics, name, case, scene):
    """16,384 rays (the specials of S.inputs among them), every lane:
    * origins within 2 K32 units of the restatement at the GPU's own directions, and the two
      frame-independent invariants within twice the fp32 oracle's (test_sampling_shapes_cpu);
    * weights at the GPU's own rays as test_gpu_parity.test_sample_ray_weights_parity builds them
      (the fp64 oracle on the fp32 sun direction, as the sweep test has it);
    * spectral: wavelengths within 1e-5 of the adopted-state oracle's and inside [360, 720];
    * w_sky = 0 and 1 (jit semantics): every pick on one side; everything finite."""
    c = ray_case(variant, precision, semantics, name, scene)
    em, o32, o64, rd, lam, gw, s3 = c.em, c.o32, c.o64, c.rd, c.lam, c.gw, c.s3
    what = f"{variant} {precision} {semantics} {name} {scene}"
    assert np.isfinite(c.ro).all() and np.isfinite(rd).all() and np.isfinite(gw).all() and np.isfinite(lam).all(), what
    misses = []

    def expect(ok, msg):
        if not ok:
            misses.append(msg)

    area = np.pi * c.radius ** 2
    # origins
    ref = o32.sample_ray(c.ws, c.s2, s3)
    fig32 = R.ray_figures(ref["o"], ref["d"], c.s2, c.center, c.radius)
    try:
        R.assert_ray_bounds(R.ray_figures(c.ro, rd, c.s2, c.center, c.radius), fig32, what)
    except AssertionError as e:
        misses.append(str(e).splitlines()[0])
    # weights at the GPU's own rays
    pdf, wrap = R.pdf_reference(o32, -rd, c.gp, c.d.get("to_world"))
    expect(wrap.sum() <= 2, f"{int(wrap.sum())} lanes on the azimuth wrap")
    # Sun picks skip the cone test (sunsky.cpp:720) and pdf_direction does not, so a sun pick compares
    # with pdf_direction where the oracle's own fp32 cone test puts it inside (its pdf then carries
    # (1 - w) sun_pdf, >= 1e4 against a sky pdf of 0.1-100).  The few sun picks a fraction of an ulp
    # outside that test (test_gpu_parity._independently_staged_sampling has the figures and the cap)
    # are not left out: their sampled pdf is held to the oracle's sampled pdf of the same sample at
    # 1e-5 and divides their reference weights.
    w_o = float(c.w_sky)
    sun_pick = s3[:, 0] >= c.w_sky
    edge = sun_pick & (pdf < 0.5 * (1.0 - w_o) / (2.0 * np.pi * (1.0 - o32.info()["cos_cutoff"])))
    expect(edge.sum() <= max(4, 5e-3 * sun_pick.sum()), f"{int(edge.sum())} sun picks outside the fp32 cone test")
    if edge.any():
        sampled = o32.sample_direction(s3, wavelengths=lam.T if variant == "spectral" else None)["pdf"]
        expect(max_rel(c.gp[edge], sampled[edge]) < 1e-5, f"edge sun picks' pdf {max_rel(c.gp[edge], sampled[edge]):.2e} off")
        pdf = np.where(edge, c.gp, pdf)
    pdf = pdf / area
    if variant == "spectral":
        rel = np.abs(lam.astype(np.float64) - ref["wavelengths"]) / ref["wavelengths"]
        print(f"RAYLAM | {what} | max rel {rel.max():.2e}, range {lam.min()!r} .. {lam.max()!r}")
        expect(rel.max() <= 1e-5, f"wavelengths {rel.max():.2e} off the oracle's")
        expect(lam.min() >= 360 and lam.max() <= 720, "wavelengths outside [360, 720]")
        _, ew32 = o32.sample_wavelengths(rd, c.ws)
        e64 = o64.eval(rd, lam.T).T
        with np.errstate(all="ignore"):
            a, b = ew32 / pdf[:, None], e64 / lambda_pdf(o64, lam) / pdf[:, None]
    else:
        expect(not lam.any(), "RGB wavelengths are not zero")
        with np.errstate(all="ignore"):
            a, b = o32.eval(rd) / pdf[:, None], o64.eval(rd) / pdf[:, None]
    sun = o32.info()["sun_dir_world"]
    cut = o32.info()["cos_cutoff"]
    margin = -rd.astype(np.float64) @ sun - cut
    lanes = margin >= -1e-6                                     # helpers.disc_lanes in the world frame
    same_formula = pdf > 0
    if same_formula.any():
        try:
            assert_parity(gw[same_formula], a[same_formula].astype(np.float32), b[same_formula], lanes[same_formula],
                          rtol=1e-5, precision=precision, sun_rtol=2e-5 if precision == "reference" else 1e-5)
        except AssertionError as e:
            misses.append("weights: " + str(e).splitlines()[0][:300])
            flip = mask_flip_lanes(a, b) & same_formula
            for i in np.nonzero(flip)[0][:4]:
                print(f"FLIP | {what} | lane {i} s3 {s3[i]!r} rd {rd[i]!r} margin {margin[i]:.3e} gpu {gw[i]!r} o32 {a[i]!r} o64 {b[i]!r} "
                      f"gp {c.gp[i]:.6e} pdf {pdf[i] * area:.6e}")
    if semantics == "jit" and name in ("sweep5", "sweep6"):
        expect(c.w_sky == (0.0 if name == "sweep5" else 1.0), f"w_sky {c.w_sky!r}")
        if c.w_sky == 0:
            expect((margin >= -1e-6).all(), "a ray from outside the disc at w_sky = 0")
        else:
            expect((s3[:, 0] < c.w_sky).all(), "a sun pick at w_sky = 1")
    assert not misses, what + ": " + "; ".join(misses)


# ---------------------------------------------------------------- 6
def test_sampling_outputs_do_not_depend_on_the_grid(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 walks 2.5 grid-stride steps (plus 3 samples)
    through the call shapes gpu_grid_stride_worker.py leaves out (W.run_grid): the masked general
    kernels prefetch the next step's mask and it.p."""
    n, n_vec = W.batch_sizes()
    env = dict(os.environ, SUNSKY_AMD_BLOCKS_PER_CU="1")
    # a child that fails or hangs fails the test here, before any GPU work of this process
    r = subprocess.run([sys.executable, W.__file__, str(n), str(n_vec), str(tmp_path)], env=env, timeout=180,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    # blocks x samples per block per step: 256 for the one-sample-per-lane kernels, 4 x 256 for pdf_direction's
    assert n > 2 * W.cap_step() and n_vec > 2 * 4 * W.cap_step()
    for variant, precision in W.COMBOS:
        path = tmp_path / f"{variant}_{precision}.npz"
        with np.load(path) as stepped:
            single = W.run_grid(variant, precision, n, n_vec)
            assert sorted(stepped.files) == sorted(single)
            for name, a in single.items():
                assert_same_bits(a, stepped[name], f"{variant} {precision} {name}")
        path.unlink()


# ---------------------------------------------------------------- 7
@VP
def test_batch_is_a_prefix_of_a_longer_batch(variant, precision):
    """m samples == the first m columns of 4099, for the call shapes test_gpu_edge_sizes.py (sizes
    0..7) and the sorted-against-unsorted tests (unmasked) leave out: masked sample_direction,
    nlam != 4 (LEAN, general, masked), partial pointer sets, masked and spectral sample_ray, masked
    pdf_direction and sample_wavelengths."""
    em = emitter(variant, precision)
    inp = inputs(variant, precision, "rotated", S.PREFIX_N)
    mk = S.mask("mixed", S.PREFIX_N)

    def calls(i, m):
        out = {"direction masked": W.sample_direction(em, i, 4, m, True, True, True),
               "direction it_p only": W.sample_direction(em, i, 4, None, True, False, False),
               "direction ds_dist only": W.sample_direction(em, i, 4, None, False, True, False),
               "direction ds_p masked": W.sample_direction(em, i, 4, m, False, False, True),
               "ray masked": W.sample_ray(em, i, m), "pdf masked": W.pdf_direction(em, i, m),
               "wavelengths masked": W.sample_wavelengths(em, i, m)}
        if variant == "spectral":
            out["ray"] = W.sample_ray(em, i)
            for nlam in (3, 8):
                out[f"LEAN nlam={nlam}"] = W.sample_direction(em, i, nlam)
                out[f"general nlam={nlam}"] = W.sample_direction(em, i, nlam, None, True, True, True)
                out[f"masked nlam={nlam}"] = W.sample_direction(em, i, nlam, m, True, True, True)
        return {k: v[0] for k, v in out.items()}

    full = calls(inp, mk)
    for m in S.PREFIX_M:
        part = calls(W.head(inp, m), mk[:m])
        for name, planes in part.items():
            same(planes, {k: v[:, :m] for k, v in full[name].items()}, f"{name} m={m}")
