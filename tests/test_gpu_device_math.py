"""The FAST device math of csrc/sunsky_kernels.hip, primitive by primitive, on the GPU over every
fp32 argument of its domain (or the dense cover its docstring states) against fp64.

tests/cpp/math_probe.hip includes the product's translation unit and calls the primitives by
name; its sweep kernels compute the fp64 reference with the device's double libm in the same
thread and reduce the worst error per block.  tests/math_probe.py re-derives each sweep's verdict
with mpmath at every block's reported worst argument, at an edge list and at 4096 random
arguments (confirm).  Bounds are the project's stated figures (source comments, DESIGN,
tools/fit_*.py) or, where none is stated, derived in the docstring from the 1e-5 parity bar of the
output the primitive feeds: the bar divided by the number of primitives feeding that output,
through the callers' first-order sensitivity.  One fp32 ulp is at most 2^-23 relative, so a
relative budget r allows r / 2^-23 ulp.  Measured values: DESIGN section 6 "Device math
primitives", profiles/device_math_measure.log (tools/device_math_measure.py)."""
import numpy as np
import pytest

import math_probe as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = P.Probe()
    yield p
    p.close()


def run_case(probe, name):
    """Sweep the case, print its figures, confirm them with mpmath, assert its bounds."""
    case = P.CASES[name]
    prim = P.PRIMS[case.prim]
    s = probe.sweep(prim.kernel, case.ranges)
    print(f"{name} | {case.domain} | {s.line()}")
    c = P.confirm(probe, case.prim, s, case.ranges)
    print(f"  mpmath at {c.checked} arguments: max ulp {c.max_ulp:.4f}, max abs {c.max_abs:.4e}")
    assert s.visited == sum(n for _, n in case.ranges)
    assert s.bad == 0, f"{name}: {s.bad} non-finite or out-of-range results in the domain"
    if case.ulp is not None:
        assert s.max_ulp <= case.ulp and c.max_ulp <= case.ulp, f"{name}: {s.line()} exceeds {case.ulp} ulp"
    if case.ab is not None:
        assert s.max_abs <= case.ab and c.max_abs <= case.ab, f"{name}: {s.line()} exceeds {case.ab} absolute"
    return s, c


def values_at(probe, prim, bit_patterns):
    p = P.PRIMS[prim]
    return probe.values(p.fn, P.floats_of(bit_patterns))[p.out]


# ------------------------------------------------------------------ the hardware wrappers
@pytest.mark.parametrize("name", ["fast_rcp", "fast_rsq", "fast_sqrt"])
def test_hardware_wrapper_is_within_one_ulp_on_normal_arguments_and_results(probe, name):
    """fast_rcp (v_rcp_f32), fast_rsq (v_rsq_f32), fast_sqrt (v_sqrt_f32): every normal argument whose
    result is normal (rcp: 2^-126 <= |x| <= 2^126, both signs; rsq, sqrt: x >= 2^-126, whose results
    lie in [2^-64, 2^64]).  Reachable: rcp(cos_theta + 0.01) >= 0.01 on active lanes, rcp of the
    larger component in atan2_fast (normal behind compute_pdfs' mask, see
    test_atan2_fast_near_the_axes_the_diagonals_and_the_mask), sqrt / rsq of sums of squares and of
    w >= 5 in erfinv_fast.  The conductor caller (mf_smith_g1: rsq(tan^2), sqrt(1 + tan^2); mf_view: rsq of a
    squared length and of sin^2 theta, whose 0 and non-finite reciprocal it replaces by (0, 1);
    mf_sample_visible_11: sqrt(-ln ux) >= 1e-3; mf_eval's rcp of alpha and cos^2 theta) hands them
    positive normal arguments too, or rsq(+0) = inf, asserted in the special values below.
    Bound: the 1 ulp the source states for v_sqrt / v_rcp."""
    run_case(probe, name)


@pytest.mark.parametrize("name", ["fast_rcp", "fast_rsq", "fast_sqrt", "fast_exp2", "log2"])
def test_hardware_wrapper_over_all_patterns_and_special_values(probe, name):
    """All 2^32 patterns are visited (the census line: arguments with a non-finite result or
    reference, and the worst error where both are finite, subnormal results included, are
    recorded, not asserted), and the special values each call site relies on are asserted:
      rcp(+-0) = +-inf, rcp(+-inf) = +-0; rsq(+0) = inf, rsq(inf) = 0; sqrt(+-0) = +-0, sqrt(inf) = inf;
      sqrt, rsq and log2 of a negative normal are NaN (dir_terms' sq below the horizon: NaN in lanes
      whose `active` is false, selected to 0 by the callers); NaN in, NaN out;
      exp2(x) = inf from x = 128, exp2(-126) is normal, exp2(0) = 1 exactly, exp2(x) = 0 for x <= -150 and for -inf
      (tgmm_sum_fast's far gaussians underflow to a 0 term);
      log2(+0) = -inf, log2(1) = 0 exactly (erfinv_fast(0): w = 0), log2(inf) = inf.
    What subnormal arguments and results do (v_rcp / v_sqrt / v_exp / v_log are not required to keep
    them) is printed for the record; no caller reaches them."""
    prim = P.PRIMS[name]
    s = probe.sweep(prim.kernel, P.ALL_PATTERNS)
    print(f"{name} | all 2^32 patterns | {s.line()}")
    assert s.visited == 1 << 32
    e = P.edges(name)
    got = values_at(probe, name, e)
    for b, g in zip(e, got):
        print(f"  {name}({P.float_of(b)!r} [{b:#010x}]) = {float(g)!r} [{P.bits_of(g):#010x}]")
    v = dict(zip(e, got))
    inf, nan_in = np.float32(np.inf), 0x7FC00000
    one, neg_one = P.bits_of(1.0), P.bits_of(-1.0)
    if name == "fast_rcp":
        assert v[0] == inf and v[P.SIGN] == -inf and not np.signbit(v[P.INF]) and v[P.INF] == 0 and np.signbit(v[P.SIGN | P.INF])
        assert v[one] == 1 and v[neg_one] == -1 and np.isnan(v[nan_in])
    elif name == "fast_rsq":
        assert v[0] == inf and v[P.INF] == 0 and v[one] == 1 and np.isnan(v[neg_one]) and np.isnan(v[nan_in])
    elif name == "fast_sqrt":
        assert v[0] == 0 and not np.signbit(v[0]) and v[P.SIGN] == 0 and v[P.INF] == inf and v[one] == 1
        assert np.isnan(v[neg_one]) and np.isnan(v[P.SIGN | P.NORMAL_MIN]) and np.isnan(v[nan_in])
    elif name == "fast_exp2":
        assert v[P.bits_of(128.0)] == inf and v[P.INF] == inf and np.isfinite(v[P.bits_of(128.0) - 1])
        assert v[P.bits_of(-126.0)] >= np.float32(2.0 ** -126) and v[0] == 1 and v[P.SIGN] == 1 and v[one] == 2
        assert v[P.bits_of(-150.0)] == 0 and v[P.bits_of(-150.0) + 1] == 0 and v[P.SIGN | P.INF] == 0 and np.isnan(v[nan_in])
    else:
        assert v[0] == -inf and v[one] == 0 and v[P.INF] == inf and np.isnan(v[neg_one]) and np.isnan(v[nan_in])


def test_fast_exp2_within_its_share_of_the_parity_bar(probe):
    """fast_exp2 (v_exp_f32) on every float of [-126, 128), the arguments with a normal result.
    Reachable: Bl2 * r and El2 * gamma in sky_fast, -(sx^2 + sy^2) <= 0 in tgmm_sum_fast, the
    conductor's exponents; results below 2^-126 flush or denormalise with an absolute error below
    2^-126, which no caller can see.  No figure is stated, so the bound is derived.  sky_fast's value
    c1 c2 is fed by 5 primitives (fast_rcp, fast_exp2, fast_rsq, fast_sqrt, asin_half_chord): exp2's
    share of the 1e-5 bar is 2e-6 relative.  exp2 enters twice, c1 = 1 + A E1 and
    c2 = ... + Ds E2 + ...; a relative error e in both moves c1 c2 by e (|A E1 / c1| + |Ds E2 / c2|)
    <= 2 e where neither term exceeds the factor it is part of, so e <= 1e-6 = 8.39 ulp.
    tgmm_sum_fast's sum of positive terms c_h E_h (also 5 primitives: atan2_fast, theta_upper_fast,
    fast_exp2, fast_rcp, fast_sqrt) takes e once: 2e-6, the looser of the two."""
    run_case(probe, "fast_exp2")


@pytest.mark.parametrize("name", ["log2 low w", "log2 high w"])
def test_hardware_log2_within_its_share_of_erfinv_fast(probe, name):
    """__builtin_amdgcn_logf (v_log_f32) inside erfinv_fast, on every float of [2^-23, 1]: its
    argument 1 - x^2 for |x| <= 1 - 2^-23 is at least 2^-22 (1 - 2^-24).  Derived bound, absolute in
    log2: erfinv_fast may be off by 1e-5 / (3 * 2 pi) = 5.3e-7 relative (see
    test_erfinv_within_its_share_of_the_sampled_angle), shared by its three error sources (log2,
    v_sqrt, the polynomials): 1.77e-7 each.  The result's relative sensitivity to w = -ln2 log2 is
    d ln p / dw <= 0.3 for w < 5 (the source's figure; pi / 12 at w = 0) and
    1 / (2 erfinv^2 + 1) <= 0.11 for w >= 5 (erfinv >= 2.07 there), so |d log2| <= 1.77e-7 / (0.3 ln 2)
    = 8.5e-7 on [e^-5, 1] and 1.77e-7 / (0.11 ln 2) = 2.32e-6 on [2^-23, e^-5).
    The other call site, mf_sample_visible_11's -ln2 log2(ux) with ux clamped to [1e-6, 1 - 1e-6], lies
    inside the swept [2^-23, 1] (2^-23 = 1.19e-7) and is covered by the same measurement; the
    conductor caller has no parity bar of its own to derive a second bound from."""
    run_case(probe, name)


# ------------------------------------------------------------------ the fitted polynomials
def test_asin_half_chord_over_its_domain(probe):
    """asin_half_chord on every float of [0, 0.7075] (half chords never exceed sqrt(1/2); the fit
    runs to sqrt(0.5005)).  Bound: the stated 0.71 ulp; asin_half_chord(0) is exactly 0."""
    run_case(probe, "asin_half_chord")
    z = values_at(probe, "asin_half_chord", [0])
    assert P.bits_of(z[0]) == 0


@pytest.mark.parametrize("name", ["elevation_fast low", "elevation_fast high"])
def test_elevation_fast_against_asin(probe, name):
    """elevation_fast on every float of [0, 1] (cos_theta of sun-disc lanes, above the horizon)
    against fp64 asin z; results within [0, pi/2] (the kernel counts the others).  Up to the switch
    z = 0.70710678 it is asin_half_chord(z): the stated 0.71 ulp (SunDisc64's comment rounds it to
    0.7).  Above it pi/2 - 2 asin_half_chord(sqrt(0.5 - 0.5 z)) the figure cannot hold, so the
    bound is from operation counts: 0.5 - 0.5 z is exact, v_sqrt's 1 ulp (2^-23 relative) is
    amplified by a / (sqrt(1 - a^2) asin a) <= 1.055 for a <= sin(pi/8), the polynomial adds 0.71 ulp of
    p <= pi/8 (ulp 2^-25); doubled, plus the final fma's rounding (2^-24) and the fp32 pi/2's error
    (4.4e-8): 2.45e-7 absolute = 4.11 ulp of a result in [pi/4, pi/2]."""
    run_case(probe, name)


def test_elevation_fast_has_no_jump_at_its_switch(probe):
    """Across z = 0.70710678 the step of elevation_fast follows the step of asin within the two
    sides' bounds (0.71 ulp below, 4.11 ulp above; ulp 2^-24 at pi/4)."""
    b = P.bits_of(P.SWITCH_Z)
    pats = [b - 1, b, b + 1, b + 2]
    got = values_at(probe, "elevation_fast", pats).astype(np.float64)
    ref = [P.REF["asin"](P.float_of(p)) for p in pats]
    for k in range(3):
        jump = abs((got[k + 1] - got[k]) - float(ref[k + 1] - ref[k])) / 2.0 ** -24
        print(f"elevation_fast step {pats[k]:#x} -> {pats[k + 1]:#x}: off by {jump:.3f} ulp")
        assert jump <= 0.71 + P.ELEVATION_HIGH_ULP


def test_atan_unit_over_its_domain(probe):
    """atan_unit on every float of [0, 1] (t = min / max, clamped to 1).  The source stated 1.07 ulp,
    from tools/fit_atan.py's 4M sampled points; every float on gfx950 gives 1.0834 ulp (at
    0x3f61f2fc), so the comment was optimistic and now carries the measured figure.  Asserted: the
    bound derived from its only caller.  atan2_fast states 4.4 ulp; in the first octant it is
    atan_unit(t) with t = min * v_rcp(max), which carries the reciprocal's ulp and the product's
    half: 1.5 ulp of t, at most 3 * 2^-24 relative, and atan does not amplify a relative error
    (t / ((1 + t^2) atan t) <= 1): 3 ulp of the result.  atan_unit may therefore use 4.4 - 3 = 1.4 ulp."""
    run_case(probe, "atan_unit")


# ------------------------------------------------------------------ atan2_fast
ATAN2_ULP, ATAN2_ABS = 4.4, 3.5e-7


def check_two_argument(probe, name, kernel, count, ulp, ab, confirm):
    s = probe.sweep(kernel, [(0, count)])
    print(f"{name} | {s.line()}")
    c = confirm(s)
    print(f"  mpmath at {c.checked} arguments: max ulp {c.max_ulp:.4f}, max abs {c.max_abs:.4e}")
    assert s.bad == 0, f"{name}: {s.bad} results non-finite, out of range or of the wrong sign"
    assert s.max_ulp <= ulp and c.max_ulp <= ulp, f"{name}: {s.line()} exceeds {ulp} ulp"
    assert s.max_abs <= ab and c.max_abs <= ab, f"{name}: {s.line()} exceeds {ab} absolute"
    return s


def test_atan2_fast_in_all_octants(probe):
    """atan2_fast(y, x) at (x, y) = (1, t) for every float t of [0, 1], in all 8 sign and swap octants
    (each octant in full, not strided): the azimuth of any direction is one of these up to the
    scale of its larger component.  Bounds: the stated 4.4 ulp and 3.5e-7 absolute; the kernel counts
    results outside [-pi, pi] (the fp32 pi) or whose sign is not y's, y = +-0 with x < 0 included."""
    def confirm(s):
        rep = s.reported()
        rng = np.random.default_rng(5)
        extra = [P.encode_atan2_octant(o, t) for o in range(8) for t in (0, 1, P.SUBNORMAL_MAX, P.NORMAL_MIN, P.BELOW_ONE - 1, P.BELOW_ONE)]
        extra += [P.encode_atan2_octant(o, t) for o, t in zip(rng.integers(0, 8, P.N_RANDOM), rng.integers(0, P.UNIT_FLOATS, P.N_RANDOM))]
        pairs = [P.decode_atan2_octant(i) for i in [a for a, _, _ in rep] + extra]
        got = probe.values(P.FN_ATAN2, [p[0] for p in pairs], [p[1] for p in pairs])[0]
        return P.confirm_pairs("atan2_fast", rep, pairs, got, P.REF["atan2"], s)
    check_two_argument(probe, "atan2_fast octants", "atan2_octant", 8 * P.UNIT_FLOATS, ATAN2_ULP, ATAN2_ABS, confirm)


def test_atan2_fast_on_scaled_circles(probe):
    """atan2_fast on the unit circle at 2^24 angles, scaled by 2^e for e = 0, -4, ..., -60 (the
    kernel's circle_point; directions whose horizontal part is short).  Same bounds."""
    def confirm(s):
        rep = s.reported()
        idx = [a for a, _, _ in rep] + list(np.random.default_rng(6).integers(0, 16 << 24, P.N_RANDOM))
        y, x = probe.values(P.FN_CIRCLE_POINT, *P.split_index(idx))
        got = probe.values(P.FN_ATAN2, y, x)[0]
        return P.confirm_pairs("atan2_fast", rep, list(zip(y, x)), got, P.REF["atan2"], s)
    check_two_argument(probe, "atan2_fast circles", "atan2_circle", 16 << 24, ATAN2_ULP, ATAN2_ABS, confirm)


def atan2_edge_pairs():
    """(y, x): |x| and |y| within 4 ulp of each other at four magnitudes; each component within 4 ulp
    of 0 (subnormals included) beside a component of 1, 2^-60 and 2^-74; all sign combinations.  2^-74
    is the smallest larger component compute_pdfs' mask `sin_theta != 0` can let through:
    sin_theta^2 = fma(x, x, y * y) is 0 in fp32 below 2^-74.5 (and a v_sqrt that flushes subnormal
    arguments zeroes it below 2^-63), so the larger component is always normal."""
    pairs = []
    for m in (1.0, 0.333, 2.0 ** -60 * 1.7, 2.0 ** -74):
        b = P.bits_of(m)
        for d in range(-4, 5):
            pairs.append((P.float_of(b + d), P.float_of(b)))
            pairs.append((P.float_of(b), P.float_of(b + d)))
    for big in (1.0, 2.0 ** -60, 2.0 ** -74):
        for small in range(0, 5):
            pairs.append((P.float_of(small), big))
            pairs.append((big, P.float_of(small)))
        for small in (2.0 ** -100, 2.0 ** -126, 2.0 ** -75):
            pairs.append((small, big))
            pairs.append((big, small))
    out = []
    for y, x in pairs:
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                out.append((np.float32(sy * y), np.float32(sx * x)))
    return out


def test_atan2_fast_near_the_axes_the_diagonals_and_the_mask(probe):
    """atan2_fast on atan2_edge_pairs against mpmath: the stated 4.4 ulp and 3.5e-7, in [-pi, pi] with
    y's sign.  Then, for the record, what it returns at (+-0, +-0) and with a subnormal larger
    component (v_rcp of it): the source promises only a finite value at (0, 0), and
    tests/test_device_math_reference_cpu.py shows from the mask that callers reach neither."""
    pairs = atan2_edge_pairs()
    got = probe.values(P.FN_ATAN2, [p[0] for p in pairs], [p[1] for p in pairs])[0]
    worst_ulp = worst_abs = 0.0
    for (y, x), g in zip(pairs, got):
        ulp, ab = P.errors(g, P.REF["atan2"](float(y), float(x)))
        worst_ulp, worst_abs = max(worst_ulp, ulp), max(worst_abs, ab)
        assert abs(g) <= np.float32(np.pi) and np.signbit(g) == np.signbit(y), (y, x, g)
        assert ulp <= ATAN2_ULP and ab <= ATAN2_ABS, (y, x, g, ulp, ab)
    print(f"atan2_fast edge pairs: {len(pairs)} | max ulp {worst_ulp:.4f} | max abs {worst_abs:.4e}")
    unreachable = [(np.float32(sy * y), np.float32(sx * x)) for y, x in ((0.0, 0.0), (1e-45, 0.0), (1e-45, 1e-45), (1e-39, 1e-40))
                   for sy in (1.0, -1.0) for sx in (1.0, -1.0)]
    got = probe.values(P.FN_ATAN2, [p[0] for p in unreachable], [p[1] for p in unreachable])[0]
    for (y, x), g in zip(unreachable, got):
        print(f"  atan2_fast({float(y)!r}, {float(x)!r}) = {float(g)!r}")
    assert np.isfinite(got[:4]).all()


def test_atan2_fast_takes_no_fixup_on_the_diagonal(probe):
    """On |y| = |x| the quotient is exactly 1 (for a power of two v_rcp is exact) and `ay > ax` is
    false: atan2_fast returns atan_unit(1) itself, pi minus it for x < 0, with y's sign, bit for bit.
    atan_unit(1) is 1 ulp below the fp32 pi/4, so taking the pi/2 - a fix-up there instead would move
    the result by 2 ulp, inside every accuracy bound above; this pins the branch."""
    a1 = probe.values(P.FN_ATAN, np.ones(1, np.float32))[0][0]
    print(f"atan_unit(1) = {float(a1)!r} [{P.bits_of(a1):#010x}], fp32 pi/4 = {P.bits_of(np.pi / 4):#010x}")
    m = np.array([1.0, 0.5, 2.0 ** -60, 2.0 ** 20, 2.0 ** -100], np.float32)
    for sy in (1, -1):
        for sx in (1, -1):
            got = probe.values(P.FN_ATAN2, sy * m, sx * m)[0]
            want = np.float32(sy) * (a1 if sx > 0 else np.float32(np.pi) - a1)
            assert (got.view(np.uint32) == np.full_like(got, want).view(np.uint32)).all(), (sy, sx, got, want)


# ------------------------------------------------------------------ sincos_fast
@pytest.mark.parametrize("name", ["sincos_fast sin", "sincos_fast cos", "sincos_fast sin, |sin| > 1e-3", "sincos_fast cos, |cos| > 1e-3"])
def test_sincos_fast_over_eight_pi(probe, name):
    """sincos_fast on every float with |x| <= 8 pi, both outputs.  Reachable: theta in [0, pi/2];
    phi = the TGMM azimuth, truncated to [0, 2 pi], plus sun_phi - pi/2 with |sun_phi| <= 2 pi, so
    |phi| <= 4.5 pi (tests/test_device_math_reference_cpu.py checks the table's means); the
    concentric disk's phi in [-pi/4, 3 pi/4].  The source stated 1.5 ulp and 9.2e-8 absolute, from
    tools/fit_sincos.py's 8M sampled points (the ulp figure for |value| > 1e-3 only: next to a zero
    of the function an absolute 1e-7 is many ulp of the value).  Every float on gfx950 gives
    9.18e-8 (sin) and 9.32e-8 (cos) absolute, 1.54 and 1.56 ulp where |value| > 1e-3, 5.79 ulp
    overall: the comment was optimistic and now carries the measured figures.  The callers' bar is
    absolute (a unit direction's components, cos(phi) sin(theta) ..., within sample_sky's share
    1e-5 / 3: 1.67e-6 on each sine or cosine, two per component), far above either figure, so the
    function stays.  Asserted: the absolute bound from operation counts, 1.07e-7, on both outputs
    (either polynomial serves either output).  Reduction: x - k C1 is exact, - k C2 rounds r to
    half an ulp (2^-25 for r in [1/2, pi/4]), times the derivative.  Cosine path: 0.707 * 2^-25 from
    r, 2^-24 relative on r2 into r2 / 2 (1.84e-8), the rounding of 1 - r2 / 2 (2^-25), 7 roundings
    on the r2^2 C term of at most 0.016 (6.6e-9), the last fma's 2^-25, the polynomial's
    truncation 5e-10: 1.062e-7.  Sine path: 0.878 * 2^-25, 6 roundings on the r^3 S term of at most
    0.081 (2.9e-8), the last fma's 2^-25, truncation 2.6e-9: 8.7e-8.
    The |value| > 1e-3 cases assert an ulp bound, 2.25, from the same counts in relative terms (an
    error of rho * 2^-24 relative is at most rho ulp).  Sine path, |value| <= 0.7072: the rounding
    of r is 2^-24 relative to r and r cos r / sin r <= 1 carries it to the sine (1.0); the r^3 S
    term is at most r^2 / 6 of the result with 6 roundings, r^2 (r / sin r) <= 0.69; truncation
    2.6e-9 of 0.707 (0.06); the reduction constants' residue, 16 * 1.8e-15, against |value| > 1e-3
    (0.0005, the reason for the qualifier: nearer a zero it is not small); the last fma's half
    ulp: 0.5 + 1.75 = 2.25.  Cosine path, value in [0.707, 1]: the 1.062e-7 above over the binade's
    ulp 2^-24: 1.78.  So a result of 0.01 that is 40 ulp off (4e-8 absolute) fails here."""
    run_case(probe, name)


def test_sincos_fast_symmetry_and_origin(probe):
    """sincos_fast(0) is exactly (0, 1); sin(-x) = -sin(x) and cos(-x) = cos(x) in bits for every
    float x of (0, 8 pi].  At x = 0 itself the sine's zero does not carry the argument's sign:
    sincos_fast(-0) is (+0, 1) (k = -0, and fma(+0, C1, -0) is +0), recorded and pinned here; the
    callers multiply it into a direction component whose zero's sign nothing reads."""
    s, c = probe.values(P.FN_SINCOS, np.array([0.0, -0.0], np.float32))
    assert P.bits_of(s[0]) == 0 and c[0] == 1
    print(f"sincos_fast(-0.0) = ({float(s[1])!r}, {float(c[1])!r})")
    assert P.bits_of(s[1]) == 0 and c[1] == 1
    first, count = P.span(0.0, P.EIGHT_PI)
    r = probe.sweep("sincos_parity", [(first + 1, count - 1)])
    print(f"sincos_fast parity | {r.line()}")
    assert r.bad == 0 and r.max_ulp == 0 and r.visited == count - 1, f"{r.bad} mismatches, one at {r.max_ulp_arg:#x}"


# ------------------------------------------------------------------ erfinv
@pytest.mark.parametrize("name", ["erfinv_fast", "erfinvf_"])
def test_erfinv_within_its_share_of_the_sampled_angle(probe, name):
    """erfinv_fast, and erfinvf_ compiled for the device, on every float of [-(1 - 2^-23), 1 - 2^-23],
    the image of 2 s - 1 for s in [kEpsilon, kOneMinusEpsilon], against fp64 erfinv.  Derived bound:
    sample_sky's direction is fed by 3 primitives (div_by_rcp, erfinv, sincos), so erfinv's share of
    the 1e-5 bar on a unit direction is 3.3e-6 on the angle sqrt(2) sigma erfinv(x) + mu (a direction
    moves by at most the angle's error).  The sample is truncated to [0, 2 pi] (azimuth) or
    [0, pi/2] and mu lies inside, so sqrt(2) sigma |erfinv x| <= 2 pi for every sigma of the table (the
    largest, 6.0, reaches it at |erfinv x| = 0.74): the angle's error is at most 2 pi times erfinv's
    relative error, which therefore may be 3.3e-6 / (2 pi) = 5.3e-7 = 4.45 ulp.
    The sequence sampler (kernels/sequence_sampling.h) has no erfinv.  The conductor caller's
    mf_sample_visible_11 calls it twice more: on 2 uy - 1 with uy clamped to [1e-6, 1 - 1e-6], inside
    this domain, and on the Newton iterate x of its slope equation, which starts in
    [-1, maxval] and which nothing clamps: an iterate with |x| >= 1 gives +-inf or NaN in
    erfinv_fast and in erfinvf_ alike (log of 0 or of a negative number; recorded by
    test_erfinv_fast_is_odd_and_continuous_at_its_switch at +-1), as in the form it restates.  Those
    arguments are outside what this test bounds."""
    run_case(probe, name)


def test_erfinv_fast_against_the_libm_log_form(probe):
    """erfinv_fast against erfinvf_ on the same domain: the source's "stays at the 1e-7 level",
    written down as twice the 1.77e-7 relative share of one error source (the two forms differ in
    the logarithm and the square root only): 3.5e-7 = 2.97 ulp."""
    s = probe.sweep("erfinv_pair", P.CASES["erfinv_fast"].ranges)
    print(f"erfinv_fast vs erfinvf_ | {s.line()}")
    args = [a for a, _, _ in s.reported()] + [int(b) for b in P.random_bits("erfinv_pair", P.CASES["erfinv_fast"].ranges)]
    fast, ref = probe.values(P.FN_ERFINV, P.floats_of(args))
    worst = max(P.errors(f, float(r))[0] for f, r in zip(fast, ref))
    print(f"  host at {len(args)} arguments: max {worst:.4f} ulp")
    assert abs(worst - s.max_ulp) <= P.AGREE_ULP
    assert s.bad == 0 and s.max_ulp <= P.ERFINV_PAIR_ULP


def test_erfinv_fast_is_odd_and_continuous_at_its_switch(probe):
    """erfinv_fast(-x) = -erfinv_fast(x) in bits on every float of [0, 1 - 2^-23]; across the switch
    w = 5 (x = sqrt(1 - e^-5)) its step follows erfinv's within twice the bound; erfinv_fast(+-1) is
    printed for the record (the samplers clamp s away from it)."""
    first, count = P.span(0.0, P.ERFINV_MAX)
    r = probe.sweep("erfinv_odd", [(first, count)])
    print(f"erfinv_fast oddness | {r.line()}")
    assert r.bad == 0 and r.max_ulp == 0 and r.visited == count, f"{r.bad} mismatches, one at {r.max_ulp_arg:#x}"
    b = P.bits_of(np.sqrt(1 - np.exp(-5.0)))
    pats = list(range(b - 3, b + 4))
    got = values_at(probe, "erfinv_fast", pats).astype(np.float64)
    ref = [P.ref_erfinv(P.float_of(p)) for p in pats]
    for k in range(len(pats) - 1):
        jump = abs((got[k + 1] - got[k]) - float(ref[k + 1] - ref[k])) / float(P.ulp_size(ref[k]))
        print(f"erfinv_fast step {pats[k]:#x} -> {pats[k + 1]:#x}: off by {jump:.3f} ulp")
        assert jump <= 2 * P.ERFINV_ULP
    ends = values_at(probe, "erfinv_fast", [P.bits_of(1.0), P.bits_of(-1.0)])
    print(f"erfinv_fast(1) = {float(ends[0])!r}, erfinv_fast(-1) = {float(ends[1])!r}")


# ------------------------------------------------------------------ the assembled angles
def test_theta_upper_fast_against_the_fp64_chord(probe):
    """theta_upper_fast at 2^24 unit directions of the upper hemisphere (z = (j + 1/2) / 4096, 4096
    azimuths) and 2 x 256 rings of 4096 azimuths within 1e-3 of the zenith and of the horizon,
    against fp64 2 asin(|v - e_z| / 2) of the same fp32 vector (acos z in its stable form).  Bound from
    operation counts: dz = z - 1 (2^-24), three roundings of the sum of squares (3 * 2^-24) and dz's
    doubled: 5 * 2^-24 on the sum, halved by the root, plus v_sqrt's 2^-23: 4.5 * 2^-24 on the half
    chord; asin amplifies a relative error by h / (sqrt(1 - h^2) asin h) <= 1.273 (h = sqrt(1/2)) and
    adds its 0.71 ulp (1.42 * 2^-24): 7.15 * 2^-24 relative, at most 7.15 ulp."""
    def confirm(s):
        rep = s.reported()
        idx = [a for a, _, _ in rep] + list(np.random.default_rng(7).integers(0, (1 << 24) + (2 << 20), P.N_RANDOM))
        lo, hi = P.split_index(idx)
        vx, vy = probe.values(P.FN_THETA_XY, lo, hi)
        vz, theta = probe.values(P.FN_THETA_Z, lo, hi)
        return P.confirm_pairs("theta_upper_fast", rep, list(zip(vx, vy, vz)), theta, P.ref_chord_angle, s)
    check_two_argument(probe, "theta_upper_fast", "theta_upper", (1 << 24) + (2 << 20), P.CHORD_ANGLE_ULP, np.inf, confirm)


def dir_confirm(probe, s, cos):
    rep = s.reported()
    idx = [a for a, _, _ in rep] + list(np.random.default_rng(8).integers(0, 3 << 21, 1024))
    lo, hi = P.split_index(idx)
    wx, wy = probe.values(P.FN_DIR_WO_XY, lo, hi)
    wz, gamma = probe.values(P.FN_DIR_WO_Z, lo, hi)
    sx, sz = probe.values(P.FN_DIR_SUN, lo, hi)
    cg, _ = probe.values(P.FN_DIR_COS, lo, hi)
    c = P.Confirmed()
    for k in range(len(idx)):
        sn, wo = (sx[k], np.float32(0), sz[k]), (wx[k], wy[k], wz[k])
        # the fp32 dot3 of the product: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), each step rounded once
        d = np.float32(np.float64(sn[2]) * np.float64(wo[2]) + np.float64(np.float32(np.float64(sn[0]) * np.float64(wo[0]))))
        ref = P.ref_dir_terms(sn, wo, bool(np.signbit(d)))[1 if cos else 0]
        ulp, ab = P.errors((cg if cos else gamma)[k], ref)
        if k < len(rep):
            # cos gamma is judged in absolute terms: next to gamma = pi/2 its ulp is that of a vanishing
            # reference, where the fp64 1 - 2 h^2 itself is only good to 1e-16 absolute
            P._agree("dir_terms", rep[k][0], None if cos else rep[k][1], rep[k][2], ulp, ab, 1.0 if cos else ref)
        c.add(idx[k], ulp, ab)
    return c


def test_dir_terms_gamma_and_cos_gamma(probe):
    """dir_terms<true>'s gamma and cos gamma for suns at 0.1, 30 and 89.5 degrees of elevation: wo at
    2^20 hemisphere points, on 128 rings of 4096 azimuths at gamma from 1e-6 to the disc edge, on 64
    rings around gamma = pi/2 (d changes sign across them) and on 64 approaching gamma = pi; against
    fp64 of the same chord form on the same fp32 vectors.  Bounds from operation counts.  Near side
    (d >= 0): the three differences round once (2 * 2^-24 on the sum of squares), its three roundings
    and v_sqrt as for theta_upper_fast: 7.15 ulp, asserted on the near rings.  Far side pi - t: t's
    error (7.15 * 2^-24 * pi/2), the subtraction's rounding (2^-23) and the fp32 pi's error
    (8.75e-8): 8.8e-7 absolute, asserted everywhere.  cos gamma = 1 - 2 h^2: h^2 carries twice h's
    4.5 * 2^-24 and its own rounding, times 2 h^2 <= 1, plus the fma's rounding: 11 * 2^-24 = 6.6e-7."""
    s = probe.sweep("dir_gamma", [(0, 3 << 21)])
    print(f"dir_terms gamma | {s.line()}")
    near = probe.sweep("dir_gamma", [((k << 21) + (1 << 20), 1 << 19) for k in range(3)])
    print(f"dir_terms gamma, rings 1e-6 .. 4.65e-3 | {near.line()}")
    sc = probe.sweep("dir_cos_gamma", [(0, 3 << 21)])
    print(f"dir_terms cos gamma | {sc.line()}")
    cg, cn, cc = dir_confirm(probe, s, False), dir_confirm(probe, near, False), dir_confirm(probe, sc, True)
    print(f"  mpmath: gamma {cg.max_abs:.4e} abs, near {cn.max_ulp:.4f} ulp, cos gamma {cc.max_abs:.4e} abs")
    assert s.bad == 0 and near.bad == 0 and sc.bad == 0
    assert s.max_abs <= P.GAMMA_ABS and cg.max_abs <= P.GAMMA_ABS
    assert near.max_ulp <= P.CHORD_ANGLE_ULP and cn.max_ulp <= P.CHORD_ANGLE_ULP
    assert sc.max_abs <= P.COS_GAMMA_ABS and cc.max_abs <= P.COS_GAMMA_ABS


def test_dir_terms_branches_agree_at_signed_zero_dot(probe):
    """dir_terms picks the chord's side by signbit(d) but gamma's and cos gamma's branch by d >= 0, which
    is true for -0: at d = -0 it forms the far chord |wo + n| and then treats it as the near one.
    That is right only because at d = 0 the two chords are equal.  Pinned here: with the sun at the
    zenith, wo = (a, b, +0) has d = +0 and wo = (-a, -b, -0), a, b > 0, has d = -0 (every product and
    sum of dot3 is -0); the two give the same gamma (pi/2) and cos gamma bit for bit.  A `signbit`
    in the second place, or a `>=` in the first, would show as pi - gamma or -cos gamma."""
    rng = np.random.default_rng(9)
    ang = 0.05 + rng.random(64) * (np.pi / 2 - 0.1)   # a, b > 0
    a, b = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    gp, cp = probe.values(P.FN_DIR_ZERO_DOT, a, b)
    gm, cm = probe.values(P.FN_DIR_ZERO_DOT, -a, -b)
    assert (gp.view(np.uint32) == gm.view(np.uint32)).all() and (cp.view(np.uint32) == cm.view(np.uint32)).all()
    assert (a > 0).all() and (b > 0).all()
    assert np.abs(gp.astype(np.float64) - np.pi / 2).max() <= P.GAMMA_ABS + 2.0 ** -23   # |wo|^2 is within 2^-23 of 1


# ------------------------------------------------------------------ the exact division
@pytest.mark.parametrize("part", range(4))
def test_div_by_rcp_is_the_ieee_quotient(probe, part):
    """div_by_rcp(a, b, RN(1 / b)) for every float a of [0, 1) (the fallback range |a| < 2^-100 and
    the subnormals included) and the divisors of math_probe.divisors(): 64 spread over (2^-20, 1]
    (w_sky, 1 - w_sky, pmf * norm magnitudes), the ends of that range, and b = 2^-100, the float
    below it, 2^-126 and 2^126 (the largest reciprocal the fast path takes, two that fall back, and the
    smallest normal reciprocal).  Bit-equal to the device's IEEE a / b and to the fp64 quotient
    rounded once: zero mismatches."""
    div = P.divisors()
    mine = np.arange(len(div))[part::4]
    s = probe.sweep("div_by_rcp", [(P.encode_div(j, 0), P.BELOW_ONE) for j in mine], aux=div)
    print(f"div_by_rcp, divisors {part}::4 ({len(mine)}) | {s.line()}")
    assert s.visited == len(mine) * P.BELOW_ONE
    assert s.bad == 0 and s.max_ulp == 0, f"{s.bad} mismatches, one at: divisor {div[P.decode_div(s.max_ulp_arg)[0]]!r}, a = {P.decode_div(s.max_ulp_arg)[1]!r}"
    # the host's own verdict at random and edge arguments: numpy's fp32 division is IEEE
    rng = np.random.default_rng(10 + part)
    a = np.concatenate([P.floats_of(rng.integers(0, P.BELOW_ONE, P.N_RANDOM)),
                        P.floats_of([0, 1, P.SUBNORMAL_MAX, P.NORMAL_MIN, P.bits_of(2.0 ** -100) - 1, P.bits_of(2.0 ** -100), P.BELOW_ONE - 1])])
    for j in mine:
        b = np.full_like(a, div[j])
        got, ieee = probe.values(P.FN_DIV, a, b)
        want = a / b
        assert (got.view(np.uint32) == want.view(np.uint32)).all() and (ieee.view(np.uint32) == want.view(np.uint32)).all(), div[j]


def test_wavelength_node_is_the_ieee_quotient_for_every_float(probe):
    """wavelength_node(lambda) = (lambda - 320) / 40 for all 2^32 patterns of lambda: bit-equal to the
    device's IEEE division and to the fp64 quotient rounded once (NaN counts as equal to NaN) at
    every pattern but the two infinities, where the correction fma forms inf - inf: NaN instead of
    +-inf, "an invalid coordinate either way" as the source says.  Exactly those two differ."""
    s = probe.sweep("wavelength_node", P.ALL_PATTERNS)
    print(f"wavelength_node | {s.line()}")
    assert s.visited == 1 << 32 and s.bad == 2, f"{s.bad} mismatches, one at lambda = {P.float_of(s.max_ulp_arg)!r}"
    finite = probe.sweep("wavelength_node", [(0, P.INF), (P.INF + 1, (1 << 31) - P.INF - 1), (P.SIGN, P.INF), (P.SIGN + P.INF + 1, (1 << 31) - P.INF - 1)])
    print(f"wavelength_node, infinities left out | {finite.line()}")
    assert finite.visited == (1 << 32) - 2 and finite.bad == 0 and finite.max_ulp == 0
    at_inf, ieee = probe.values(P.FN_WAVELENGTH, np.array([np.inf, -np.inf], np.float32))
    assert np.isnan(at_inf).all() and ieee[0] == np.inf and ieee[1] == -np.inf
    rng = np.random.default_rng(11)
    lam = np.concatenate([P.floats_of(rng.integers(0, 1 << 32, P.N_RANDOM)), np.array([320, 360, 720, 0, 319.99997, 1e-45], np.float32)])
    got, ieee = probe.values(P.FN_WAVELENGTH, lam)
    with np.errstate(all="ignore"):
        want = (lam - np.float32(320)) / np.float32(40)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all() and ((ieee.view(np.uint32) == want.view(np.uint32)) | np.isnan(want)).all()


# ------------------------------------------------------------------ the disk and the cone
def grid_confirm(probe, s, fn_xy, fn_z, ref):
    rep = s.reported()
    idx = [a for a, _, _ in rep] + list(np.random.default_rng(12).integers(0, 1 << 24, 1024))
    pts = [P.grid_point(i) for i in idx]
    sx, sy = [p[0] for p in pts], [p[1] for p in pts]
    x, y = probe.values(fn_xy, sx, sy)
    z = probe.values(fn_z, sx, sy)[0] if fn_z is not None else None
    c = P.Confirmed()
    for k in range(len(idx)):
        want = ref(float(sx[k]), float(sy[k]))
        got = (x[k], y[k]) if z is None else (x[k], y[k], z[k])
        ab = max(P.errors(g, w)[1] for g, w in zip(got, want))
        if k < len(rep) and rep[k][2] is not None:
            assert abs(rep[k][2] - ab) <= P.AGREE_ULP * 2.0 ** -24, (idx[k], rep[k], ab)
        c.add(idx[k], ab * 2.0 ** 24, ab)
    return c


def test_disk_concentric_fast_on_the_sample_grid(probe):
    """disk_concentric_dev<true> at (sx, sy) = (k, j) / 4096, a 4096 x 4096 grid that holds the centre, both
    axes and both diagonals |x| = |y| of (2 sx - 1, 2 sy - 1), against fp64 of the same map.  Bound from
    operation counts, absolute per component: phi = (pi/4 rp) rcp(r) carries 4.5 * 2^-24 relative
    (the constant, two products, v_rcp) of at most pi/4, then pi/2 - phi's rounding (2^-24) and
    constant (4.4e-8): 3.2e-7 on phi; sincos_fast adds its 1.07e-7 (test_sincos_fast_over_eight_pi) and
    the product with |r| <= 1 its rounding 2^-24: 4.8e-7.  |p| <= 1 holds up to rounding only (at
    |r| = 1 the point is a cosine and a sine rounded to fp32, whose squares sum above 1 about as
    often as below; 4083 of the 2^24 grid points do): the kernel counts points with px^2 + py^2
    above 1 + 4.3e-7 in fp64, the slack being 2 sqrt(2) * 1.07e-7 from the two outputs and 2^-23 from
    the two products.  What the cone needs of it, z >= cos_cutoff, is asserted without slack in
    test_uniform_cone_fast_on_the_sample_grid."""
    s = probe.sweep("disk_concentric", [(0, 1 << 24)])
    print(f"disk_concentric_dev<true> | {s.line()}")
    c = grid_confirm(probe, s, P.FN_DISK, None, P.ref_disk)
    print(f"  mpmath at {c.checked} arguments: max abs {c.max_abs:.4e}")
    assert s.max_abs <= P.DISK_ABS and c.max_abs <= P.DISK_ABS
    assert s.bad == 0, f"{s.bad} grid points outside the unit disk by more than {P.DISK_SLACK}"


@pytest.mark.parametrize("aperture", range(3))
def test_uniform_cone_fast_on_the_sample_grid(probe, aperture):
    """uniform_cone_dev<true> on the same grid at the default sun half aperture (0.2665 degrees), 5 and
    30 degrees, against fp64 of the same map with the same fp32 cos_cutoff.  Bound: the disk's 4.8e-7
    per component (x and y scale it by sc <= sin 30 degrees; z = cos_cutoff + omc (1 - pn) carries
    omc * 1.03e-6 and three roundings, 2.7e-7 at 30 degrees).  z >= cos_cutoff: the kernel counts
    the points below."""
    cc = probe.values(P.FN_CONE_Z + aperture, np.zeros(1, np.float32), np.zeros(1, np.float32))[1][0]
    s = probe.sweep("uniform_cone", [(aperture << 24, 1 << 24)])
    print(f"uniform_cone_dev<true>, cos_cutoff {float(cc)!r} | {s.line()}")
    c = grid_confirm(probe, s, P.FN_CONE_XY + aperture, P.FN_CONE_Z + aperture, lambda sx, sy: P.ref_cone(sx, sy, cc))
    print(f"  mpmath at {c.checked} arguments: max abs {c.max_abs:.4e}")
    assert s.max_abs <= P.DISK_ABS and c.max_abs <= P.DISK_ABS
    assert s.bad == 0, f"{s.bad} grid points below cos_cutoff"
