"""The eval and bake kernels at every call shape, stride and edge: sunsky_eval and
sunsky_eval_direction (RGB; spectral per-ray at every wavelength count, the rays4 kernel among
them), sunsky_eval_spectral_broadcast (one wavelength, an off-node list, the 11 nodes, 32) in their
4-directions-per-lane, one-per-lane and _dir forms, and sunsky_bake_latlong -- RGB and spectral,
both precisions, identity and a to_world rotated 0.5 rad about x.  Every eval batch holds disc
directions (every eighth), a band around the limb and directions below the horizon
(eval_shapes_reference.directions), so every shape walks the disc path and, in the FAST broadcast
and node kernels, the disc fix-up pass (fixup_spec_disc).

  1. strides, alignment and canaries through the C ABI: against the call with every plane 16-byte
     aligned and the strides n rounded up to 4 (a v4 body plus a v1 tail), each plane base in turn
     one float off alignment, the mask one byte off, ostride n + 5, lstride n + 5, packed strides
     (n), all together: the same bits, and every element outside columns [0, n) keeps its canary.
  2. masks: none, all on, all off, every third lane off, only the tail off, only the body off,
     "on" bytes 1, 2, 0x80, 0xFF; active lanes carry the unmasked call's bits, inactive lanes +0.0
     whatever direction they hold (disc, below the horizon, zero, NaN, +-Inf); a NaN, Inf or zero
     direction in one slot of a 4-direction lane leaves the other slots' bits alone; an invalid
     wavelength on a disc lane gives +0.0.
  3. wavelength counts: per-ray 1..16 against the rows of the 16-plane call, 2, 9 and 16 against
     the oracle; broadcast lists of 1, the 11 nodes, the nodes reversed and 32 against the oracle,
     each row of the 32 against a one-entry call; counts outside the range refused, nothing written.
  4. the bake against the oracle (eval_shapes_reference.BakeReference): every pixel, the horizon
     rows included, inside a bound derived from the two oracles and the device's sincosf bound.
  5. the bake's layout through the C ABI: strides, alignment, canaries, refusal.
  6. the sequence bake against the weighted sum of the per-frame references.

Bit-for-bit comparisons count two NaNs as equal and require that none appears."""
import functools
import math

import numpy as np
import pytest
import torch

import eval_shapes_reference as R
import gpu_eval_worker as W
import sequence_cases as SC
import sunsky_amd as ss
from helpers import assert_parity
from test_gpu_direct_shapes import assert_same_bits

pytestmark = pytest.mark.gpu

VPF = pytest.mark.parametrize("variant,precision,frame", R.COMBOS, ids=["-".join(c) for c in R.COMBOS])
PF = pytest.mark.parametrize("precision,frame", [(p, f) for p in ("fast", "reference") for f in R.FRAMES],
                             ids=[f"{p}-{f}" for p in ("fast", "reference") for f in R.FRAMES])
PARITY_N = 4099


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def _inputs(n, frame):
    return R.inputs(n, frame)


def _zero_bits(a, what):
    bits = np.ascontiguousarray(a).view(np.int32)
    assert not bits.any(), f"{what}: {int(np.count_nonzero(bits))} of {bits.size} values are not +0.0"


# ---------------------------------------------------------------- 1
@VPF
def test_strides_alignment_and_canaries(variant, precision, frame):
    """Every size, every entry point, every layout of gpu_eval_worker.layouts(): columns [0, n) of
    every plane equal the baseline's bits and nothing else is written.  The layouts that move the
    mask are run, like their baseline, under the every-third-lane-off mask."""
    _gpu()
    em = W.emitter(variant, precision, frame)
    for n in R.SIZES:
        inp, third = _inputs(n, frame), R.mask("third_off", n)
        for name, entry, kw in W.entries(variant):
            base = {}
            for masked in (False, True):
                base[masked], lost = W.run_entry(em, entry, kw, inp, third if masked else None)
                assert lost == 0, f"{name} n={n} baseline: {lost} elements outside columns [0, n) were written"
            for lay in W.layouts(n)[1:] + [W.Layout(ostride=n, lstride=n, name="packed")]:
                got, lost = W.run_entry(em, entry, kw, inp, third if lay.mask_off else None, lay)
                assert_same_bits(got, base[lay.mask_off], f"{name} n={n} {lay.name}")
                assert lost == 0, f"{name} n={n} {lay.name}: {lost} elements outside columns [0, n) were written"


@pytest.mark.parametrize("precision", ["fast", "reference"])
def test_single_plane_strides_do_not_matter(precision):
    """One output plane (nlam 1, m 1) or one wavelength plane: a stride is checked and used from the
    second plane on only (check_ray_strides).  Strides 0 and 7 (odd, and below n) give the packed
    bits and write one plane only; the layout is otherwise the baseline's, so the call stays on
    the 4-directions-per-lane kernels (sunsky_eval and sunsky_eval_spectral_broadcast pass 0 to
    vec4_count for a stride that is not used), which never see a second plane's offset."""
    _gpu()
    em = W.emitter("spectral", precision, "identity")
    for n in R.SIZES:
        inp = _inputs(n, "identity")
        for name, entry, kw in [e for e in W.entries("spectral") if e[0].endswith(("nlam1", "m1"))]:
            base, lost = W.run_entry(em, entry, kw, inp)
            assert lost == 0
            lays = [W.Layout(ostride=0), W.Layout(ostride=7)]
            if entry != "broadcast":
                lays += [W.Layout(lstride=0), W.Layout(lstride=7), W.Layout(ostride=7, lstride=7)]
            for lay in lays:
                got, lost = W.run_entry(em, entry, kw, inp, None, lay)
                assert_same_bits(got, base, f"{name} n={n} {lay.name}")
                assert lost == 0, f"{name} n={n} {lay.name}: {lost} elements outside the plane were written"


def test_canary_check_sees_a_write_outside_the_columns():
    """The Buf bookkeeping itself: a write into a pad column, a guard on either side and the spare
    plane is each counted."""
    _gpu()
    b = W.Buf(3, 5, 13)
    assert b.columns(2).shape == (2, 5) and b.untouched() == 0
    b.buf[b.base + 5] = 1.0            # the first pad column of plane 0
    b.buf[b.base + 2 * 13] = 1.0       # the spare plane
    b.buf[b.base - 1] = 1.0            # the last guard element in front
    b.buf[-1] = 1.0                    # the last guard element behind
    assert b.untouched() == 4


# ---------------------------------------------------------------- 2
@VPF
def test_masks(variant, precision, frame):
    """Every mask pattern at every size, aligned and with everything strided and off alignment:
    active lanes carry the unmasked call's bits, inactive lanes are +0.0 on every plane -- among
    them disc lanes (the FAST fix-up pass must not write its term over the zero) and lanes below
    the horizon.  Any non-zero byte is on."""
    _gpu()
    em = W.emitter(variant, precision, frame)
    for n in R.SIZES:
        inp = _inputs(n, frame)
        for name, entry, kw in W.entries(variant):
            for lay in (W.layouts(n)[0], W.layouts(n)[-1]):
                full, lost = W.run_entry(em, entry, kw, inp, None, lay)
                assert lost == 0 and not np.isnan(full).any()
                for kind in R.MASKS[1:]:
                    m = R.mask(kind, n)
                    got, lost = W.run_entry(em, entry, kw, inp, m, lay)
                    want = np.where(m[None, :] != 0, full, np.float32(0.0))
                    assert_same_bits(got, want, f"{name} n={n} {lay.name} mask {kind}")
                    assert lost == 0, f"{name} n={n} {lay.name} mask {kind}: {lost} elements outside were written"
        if n == 4099:
            sun = R.sun_lanes(frame, inp["wo"].T)
            assert (sun & (R.mask("third_off", n) == 0)).sum() > 100 and (sun & (R.mask("on_bytes", n) == 0)).sum() > 50


SPECIAL_AT = (5, 14, 23, 32, 41)      # slots 1, 2, 3, 0, 1 of five different 4-direction lanes


@VPF
def test_special_directions(variant, precision, frame):
    """The zero vector, NaN and +-Inf directions (eval_shapes_reference.SPECIAL_DIRS) in single slots
    of 4-direction lanes and in the one-per-lane tail.  Masked off: +0.0 there and every other
    column keeps the clean call's bits.  Unmasked: every other column keeps the clean call's
    bits, and a column whose direction is finite (the zero vector) holds no NaN."""
    _gpu()
    em = W.emitter(variant, precision, frame)
    for n in (8, 1025):
        clean = _inputs(n, frame)
        at = [p for p in SPECIAL_AT if p < n - 1] or [1, 2]
        at = at + [n - 1] if n % 4 else at + [n - 2]
        wo = clean["wo"].copy()
        specials = list(R.SPECIAL_DIRS.values())
        for k, p in enumerate(at):
            wo[:, p] = specials[k % len(specials)]
        dirty = dict(clean, wo=wo)
        finite = np.isfinite(wo).all(axis=0)
        other = np.ones(n, bool)
        other[at] = False
        m = other.astype(np.uint8)
        for name, entry, kw in W.entries(variant):
            for lay in (W.layouts(n)[0], W.layouts(n)[-1]):
                want, _ = W.run_entry(em, entry, kw, clean, None, lay)
                got, lost = W.run_entry(em, entry, kw, dirty, m, lay)
                assert lost == 0
                assert_same_bits(got[:, other], want[:, other], f"{name} n={n} {lay.name} specials masked off")
                _zero_bits(got[:, ~other], f"{name} n={n} {lay.name} masked special directions")
                got, lost = W.run_entry(em, entry, kw, dirty, None, lay)
                assert lost == 0
                assert_same_bits(got[:, other], want[:, other], f"{name} n={n} {lay.name} specials unmasked")
                assert not np.isnan(got[:, finite]).any(), f"{name} n={n} {lay.name}: NaN from a finite direction"


@PF
def test_invalid_wavelength_on_a_disc_lane(precision, frame):
    """300 nm, 800 nm and NaN give +0.0 on every lane, the disc lanes included (the FAST fix-up pass
    skips f < 0), per-ray through the rays4 and the general kernel and broadcast; the valid
    wavelength next to them lights the disc lanes."""
    _gpu()
    em = W.emitter("spectral", precision, frame)
    n = 1025
    inp = _inputs(n, frame)
    bad = [300.0, 800.0, float("nan"), 555.0]
    lam = np.repeat(np.asarray(bad + [555.0], np.float32)[:, None], n, 1)
    sun = R.sun_lanes(frame, inp["wo"].T)
    assert sun.sum() >= n // 8
    for lay in (W.layouts(n)[0], W.layouts(n)[-1]):
        calls = {"rays4": W.eval_call(em, "eval", inp["wo"], lam, 4, None, lay),
                 "rays5": W.eval_call(em, "eval", inp["wo"], lam, 5, None, lay),
                 "direction4": W.eval_call(em, "eval_direction", inp["wo"], lam, 4, None, lay),
                 "broadcast": W.eval_call(em, "broadcast", inp["wo"], bad, 0, None, lay)}
        for name, (got, lost) in calls.items():
            assert lost == 0
            _zero_bits(got[:3], f"{name} {lay.name}: planes of invalid wavelengths")
            assert (got[3][sun] > 0).all() and not np.isnan(got[3]).any(), name
        assert_same_bits(calls["rays4"][0][3], calls["broadcast"][0][3], "per-ray 555 nm against broadcast 555 nm")


# ---------------------------------------------------------------- 3
def _parity(got, variant, frame, wo, lam, precision, what):
    """assert_parity at its own bars; rotated: the sun_k = 4 rule of test_gpu_entry_points.
    got (C, n); wo (3, n) world directions; lam a list or (k, n) planes."""
    o32, o64 = R.oracles(variant, frame)
    a, b = R.oracle_eval(o32, wo.T, lam), R.oracle_eval(o64, wo.T, lam)
    print(what)
    return assert_parity(got.T, a.T, b.T, R.sun_lanes(frame, wo.T), precision=precision,
                         sun_k=4.0 if frame == "rotated" else None)


@PF
def test_per_ray_wavelength_counts(precision, frame):
    """nlam 1, 2, 3, 4 (the rays4 kernel), 5, 8, 9 (a last chunk of one plane) against the rows of
    the 16-plane call (the maximum), bit for bit, through eval and eval_direction; 2, 9 and 16
    against the oracle; 0 and 17 refused with nothing written."""
    _gpu()
    em = W.emitter("spectral", precision, frame)
    inp = _inputs(PARITY_N, frame)
    for entry in ("eval", "eval_direction"):
        full, lost = W.eval_call(em, entry, inp["wo"], inp["lam"], 16)
        assert lost == 0
        for nlam in (1, 2, 3, 4, 5, 8, 9):
            got, lost = W.eval_call(em, entry, inp["wo"], inp["lam"], nlam)
            assert lost == 0 and got.shape == (nlam, PARITY_N)
            assert_same_bits(got, full[:nlam], f"{entry} nlam={nlam} against the rows of nlam=16")
        for nlam in (2, 9, 16):
            _parity(full[:nlam], "spectral", frame, inp["wo"], inp["lam"][:nlam], precision, f"{entry} nlam={nlam}")
        for nlam in (0, 17):
            got, lost = W.eval_call(em, entry, inp["wo"], inp["lam"], nlam, expect=W.INVALID_VALUE)
            assert lost == 0, f"{entry} nlam={nlam}: refused, yet {lost} elements were written"


@PF
def test_broadcast_wavelength_counts(precision, frame):
    """m = 1, the 11 nodes (the node kernel), the nodes reversed (the general kernel) and 32
    (duplicates, nodes, 720, 719.99, 300, 800) against the oracle; each row of the 32 equals a
    one-entry call at that wavelength; the reversed nodes equal the node kernel's rows within the
    oracle's bar only (two kernels), 0 and 33 entries are refused."""
    _gpu()
    em = W.emitter("spectral", precision, frame)
    inp = _inputs(PARITY_N, frame)
    got = {}
    for name, lam in (("m1", [555.0]), ("nodes", R.NODES), ("reversed", R.NODES[::-1]), ("m32", R.LIST32)):
        got[name], lost = W.eval_call(em, "broadcast", inp["wo"], lam)
        assert lost == 0, name
        _parity(got[name], "spectral", frame, inp["wo"], lam, precision, f"broadcast {name}")
    assert len(R.LIST32) == R.MAX_BROADCAST
    single = {}
    for k, lam in enumerate(R.LIST32):
        if lam not in single:
            single[lam], lost = W.eval_call(em, "broadcast", inp["wo"], [lam])
            assert lost == 0
        assert_same_bits(got["m32"][k], single[lam][0], f"row {k} ({lam} nm) of the 32-entry list against m = 1")
    for k in (R.LIST32.index(300.0), R.LIST32.index(800.0)):
        _zero_bits(got["m32"][k], f"row {k} of the 32-entry list")
    for lam in ([], [500.0] * 33):
        _, lost = W.eval_call(em, "broadcast", inp["wo"], lam, expect=W.INVALID_VALUE)
        assert lost == 0, f"m={len(lam)}: refused, yet {lost} elements were written"


# ---------------------------------------------------------------- 4
@functools.lru_cache(maxsize=None)
def _bake_ref(variant, frame, lname, image):
    name, w, h, theta, phi, cap = next(i for i in R.bake_images(frame) if i[0] == image)
    return R.BakeReference(variant, frame, w, h, theta, phi, R.bake_lists(variant)[lname]), cap


@VPF
def test_bake_against_the_oracle(variant, precision, frame):
    """Every image of eval_shapes_reference.bake_images -- whole spheres from 1 x 1 to 64 x 33
    (w % 4 of 0, 1, 2 and 3, h == 1 and w == 1), a window, the same window with both ranges
    reversed (held to the reference of the reversed ranges, which test_eval_shapes_cpu.py shows to be
    the mirrored window), and two windows around the sun (scalar stores at w = 33, 16-byte at w = 36)
    -- inside the bound on every pixel, the horizon rows included; pixels structurally below the
    horizon exactly 0; planes of wavelengths outside the model exactly 0; under the rotation the
    rows below the image's horizon that the rotation lifts are lit."""
    _gpu()
    em = W.emitter(variant, precision, frame)
    for lname, lam in R.bake_lists(variant).items():
        for image, w, h, theta, phi, _ in R.bake_images(frame):
            ref, cap = _bake_ref(variant, frame, lname, image)
            img = em.bake_latlong(w, h, theta, phi, wavelengths=lam).cpu().numpy().reshape(-1, h * w)
            what = f"BAKE | {variant} {precision} {frame} {lname} {image}"
            ref.check(img, cap, what)
            valid = [0, 1, 2] if lam is None else [k for k, v in enumerate(lam) if 320.0 <= v <= 720.0]
            for k in set(range(img.shape[0])) - set(valid):
                _zero_bits(img[k], f"{what} plane {k}")
            if frame == "rotated":
                row_ct = np.repeat(np.cos(ref.theta.astype(np.float64)), w)
                lifted = (row_ct < 0) & (ref.o64[valid] > 0).all(axis=0)
                assert lifted.any() or not (image.startswith("sphere") and w >= 7 and h >= 5), what
                assert (img[valid][:, lifted] > 0).all(), f"{what}: lifted pixels left dark"


# ---------------------------------------------------------------- 5
@VPF
def test_bake_layout_through_the_c_abi(variant, precision, frame):
    """(8, 5), (9, 7) over the sphere and (36, 33) around the sun: ostride w h (packed; 16-byte
    stores where w % 4 == 0), w h + 5, and w h rounded up to 4 with the output one float off
    alignment carry the aligned call's bits with every canary intact; ostride < w h is refused."""
    _gpu()
    em = W.emitter(variant, precision, frame)
    for lname, lam in R.bake_lists(variant).items():
        for w, h in R.LAYOUT_SIZES:
            theta, phi = R.sun_window(frame) if (w, h) == (36, 33) else ((0.0, math.pi), (0.0, 2 * math.pi))
            base, lost = W.bake_call(em, w, h, theta, phi, lam)
            assert lost == 0
            wrapped = em.bake_latlong(w, h, theta, phi, wavelengths=lam).cpu().numpy().reshape(-1, w * h)
            assert_same_bits(wrapped, base, f"{lname} {w}x{h} the wrapper's packed call")
            for what, kw in (("packed", dict(ostride=w * h)), ("ostride+5", dict(ostride=w * h + 5)),
                             ("off alignment", dict(off=True)), ("off alignment, ostride+5", dict(ostride=w * h + 5, off=True))):
                got, lost = W.bake_call(em, w, h, theta, phi, lam, **kw)
                assert_same_bits(got, base, f"{lname} {w}x{h} {what}")
                assert lost == 0, f"{lname} {w}x{h} {what}: {lost} elements outside the image were written"
            _, lost = W.bake_call(em, w, h, theta, phi, lam, ostride=w * h - 1, expect=W.INVALID_VALUE)
            assert lost == 0


# ---------------------------------------------------------------- 6
SEQ_SIZES = [(9, 7), (37, 13), (36, 9)]


@functools.lru_cache(maxsize=None)
def _sequence_ref(variant, rotated, count, size):
    """sum_f w_f o64_f and the weighted sum of the per-frame bounds, frames of sequence_cases."""
    base = SC.base_dict(**({"to_world": SC.rotation()} if rotated else {}))
    suns = SC.frame_dirs(base.get("to_world"))[:count]
    lam = SC.LAMBDAS if variant == "spectral" else None
    o64 = bound = dark = None
    for s, t, wt in zip(suns, SC.TURBIDITY, SC.WEIGHTS):
        ref = R.BakeReference(variant, None, *size, lam=lam, d=SC.frame_dict(base, s, t))
        o64 = wt * ref.o64 if o64 is None else o64 + wt * ref.o64
        bound = wt * ref.bound if bound is None else bound + wt * ref.bound
        dark = ref.dark if dark is None else dark & ref.dark
    return o64, bound, dark


@pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])
@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_sequence_bake_against_the_oracle(variant, rotated):
    """A one-frame and a three-frame SunskySequence (the frames, turbidities and weights of
    sequence_cases) at (9, 7), (37, 13) and (36, 9): every pixel within the weighted sum of the
    per-frame bounds of sum_f w_f o64_f, pixels dark in every frame exactly 0."""
    _gpu()
    base = SC.base_dict(**({"to_world": SC.rotation()} if rotated else {}))
    em = ss.SunskyEmitter(base, variant)
    lam = SC.LAMBDAS if variant == "spectral" else None
    for count in (1, 3):
        suns = SC.frame_dirs(base.get("to_world"))[:count]
        seq = ss.SunskySequence(em, suns, SC.TURBIDITY[:count], SC.WEIGHTS[:count])
        for w, h in SEQ_SIZES:
            o64, bound, dark = _sequence_ref(variant, rotated, count, (w, h))
            img = seq.bake_latlong(w, h, wavelengths=lam).cpu().numpy().reshape(-1, w * h)
            assert not np.isnan(img).any()
            r = np.abs(img - o64) / bound
            print(f"SEQBAKE | {variant} {'rotated' if rotated else 'identity'} frames {count} {w}x{h}: worst ratio {r.max():.3f}")
            assert (r <= 1.0).all(), f"frames {count} {w}x{h}: {int((r > 1).any(axis=0).sum())} pixels over, worst {r.max():.3g}x"
            assert not img[:, dark].any()
