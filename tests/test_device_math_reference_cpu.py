"""The host side of the device-math probe (tests/math_probe.py), without a GPU: the ulp metric on
hand-made pairs, every mpmath reference against numpy / scipy fp64, the index decoders of the
two-argument sweeps, the divisor and edge lists and the swept ranges that the docstrings of
tests/test_gpu_device_math.py describe, the facts about the TGMM table and the pdf mask that
those docstrings lean on, and the probe's build rule against the product's."""
import os
import re
import struct

import numpy as np
import pytest

import math_probe as P
import sunsky_amd as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------ the metric
def test_ulp_metric_on_neighbours_binades_the_normal_floor_and_zeros():
    one_up = P.float_of(P.bits_of(1.0) + 1)       # 1 + 2^-23
    one_down = P.float_of(P.bits_of(1.0) - 1)     # 1 - 2^-24
    # neighbours: one ulp apart in the reference's binade
    assert P.errors(one_up, 1.0) == (1.0, 2.0 ** -23)
    assert P.errors(1.0, one_up) == (1.0, 2.0 ** -23)
    # across a binade: the ulp is the reference's, so the same gap counts differently from each side
    assert P.errors(1.0, one_down) == (1.0, 2.0 ** -24)
    assert P.errors(one_down, 1.0) == (0.5, 2.0 ** -24)
    assert P.errors(2.0, P.float_of(P.bits_of(2.0) - 1)) == (1.0, 2.0 ** -23)
    # a reference that is no float: 1.75 ulp below 1 + 2^-23 * 1.75
    assert P.errors(1.0, P.MP.mpf(1) + P.MP.mpf(2) ** -23 * 1.75)[0] == 1.75
    # the floor at the smallest normal: subnormal references are measured in 2^-149
    tiny = 2.0 ** -149
    assert float(P.ulp_size(2.0 ** -126)) == tiny and float(P.ulp_size(2.0 ** -140)) == tiny and float(P.ulp_size(0)) == tiny
    assert float(P.ulp_size(2.0 ** -125)) == 2 * tiny
    assert P.errors(3 * tiny, 0.0) == (3.0, 3 * tiny)
    assert P.errors(0.0, 2.0 ** -126) == (2.0 ** 23, 2.0 ** -126)
    # signed zeros are the same value; the sign of the reference does not matter
    assert P.errors(-0.0, 0.0) == (0.0, 0.0) and P.errors(0.0, -0.0) == (0.0, 0.0)
    assert P.errors(-one_up, -1.0) == (1.0, 2.0 ** -23)
    # a non-finite result is infinitely wrong
    assert P.errors(np.inf, 1.0)[0] == np.inf and P.errors(np.nan, 1.0)[0] == np.inf


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", sorted(P.REF64_DOMAIN))
def test_mpmath_reference_agrees_with_fp64(name):
    """1e4 points of the domain: the fp64 library value within 2 fp64 ulp of the 128-bit one."""
    lo, hi = P.REF64_DOMAIN[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if lo > 0 and hi / lo > 1e6:
        x = np.exp(rng.uniform(np.log(lo), np.log(hi), 10000))
    else:
        x = rng.uniform(lo, hi, 10000)
    x = x.astype(np.float32).astype(np.float64)
    lib = P.REF64[name](x)
    worst = 0.0
    for xi, li in zip(x, lib):
        ref = P.REF[name](float(xi))
        worst = max(worst, abs(float((P.MP.mpf(float(li)) - ref) / P.MP.mpf(float(np.spacing(abs(float(ref))))))))
    # scipy's erfinv is itself good to about 2.3 fp64 ulp only (2.25 at 16 of these points, where
    # mpmath's own 128-bit erfinv equals ref_erfinv to the last digit), so it is held to 3; the 2 ulp
    # the others get would test scipy, not the reference.  test_mpmath_erfinv_reference_equals_mpmaths_own_inverse
    # holds the reference tighter.
    bound = 3.0 if name == "erfinv" else 2.0
    print(f"{name}: {worst:.3f} fp64 ulp")
    assert worst <= bound, f"{name}: {worst} fp64 ulp"


def test_mpmath_erfinv_reference_equals_mpmaths_own_inverse():
    """ref_erfinv (Newton steps on erf) against mpmath's own erfinv (its root finder) at 128 bits:
    equal to 2^-110 relative at 300 points of the domain, the tails included (beside the fp64
    comparison above, which scipy's erfinv is too coarse to hold to 2 ulp)."""
    x = np.random.default_rng(2).uniform(-1, 1, 294).astype(np.float32).tolist() + [P.ERFINV_MAX, -P.ERFINV_MAX, 2.0 ** -126, 1e-45, 0.5, -0.5]
    for v in x:
        own = P.MP.erfinv(P.MP.mpf(v))
        assert abs(P.ref_erfinv(v) - own) <= abs(own) * P.MP.mpf(2) ** -110, v
    assert P.ref_erfinv(0.0) == 0 and P.ref_erfinv(1.0) == P.MP.inf and P.ref_erfinv(-1.0) == -P.MP.inf


def test_mpmath_atan2_agrees_with_fp64():
    rng = np.random.default_rng(3)
    y, x = rng.standard_normal((2, 10000)).astype(np.float32).astype(np.float64)
    for yi, xi, li in zip(y, x, np.arctan2(y, x)):
        ref = P.REF["atan2"](float(yi), float(xi))
        assert abs(float(P.MP.mpf(float(li)) - ref)) <= 2 * np.spacing(abs(float(ref)))
    assert float(P.REF["atan2"](-0.0, -1.0)) == -np.pi and float(P.REF["atan2"](0.0, -1.0)) == np.pi


def test_composite_references_agree_with_fp64():
    rng = np.random.default_rng(4)
    for sx, sy in rng.random((200, 2)).astype(np.float32):
        x, y = 2 * float(sx) - 1, 2 * float(sy) - 1
        r, rp = (y, x) if abs(x) < abs(y) else (x, y)
        phi = np.pi / 4 * rp / r
        phi = np.pi / 2 - phi if abs(x) < abs(y) else phi
        px, py = P.ref_disk(float(sx), float(sy))
        assert abs(float(px) - r * np.cos(phi)) < 1e-15 and abs(float(py) - r * np.sin(phi)) < 1e-15
        cx, cy, cz = P.ref_cone(float(sx), float(sy), np.float32(0.8660254))
        assert abs(float(cx * cx + cy * cy + cz * cz) - 1) < 1e-15 and float(cz) >= f32(0.8660254) - 1e-15
    assert P.ref_disk(0.5, 0.5) == (0, 0)
    for v in rng.standard_normal((200, 3)):
        v = (v / np.linalg.norm(v)).astype(np.float32)
        v[2] = abs(v[2])
        assert abs(float(P.ref_chord_angle(*map(float, v))) - np.arccos(np.float64(v[2]))) < 1e-6
        g, c = P.ref_dir_terms((0.0, 0.0, 1.0), v, False)
        assert abs(float(P.MP.cos(g) - c)) < 1e-30
        g, c = P.ref_dir_terms((0.0, 0.0, -1.0), v, True)
        assert abs(float(P.MP.cos(g) - c)) < 1e-30 and float(g) >= np.pi / 2 - 1e-6


# ------------------------------------------------------------------ the decoders
def test_pair_decoders_round_trip():
    rng = np.random.default_rng(1)
    for octant in range(8):
        for tbits in [0, 1, P.BELOW_ONE - 1, P.BELOW_ONE] + list(rng.integers(0, P.UNIT_FLOATS, 50)):
            idx = P.encode_atan2_octant(octant, tbits)
            assert idx < 8 * P.UNIT_FLOATS
            y, x = P.decode_atan2_octant(idx)
            big, small = (y, x) if octant & 1 else (x, y)
            assert abs(big) == 1 and P.bits_of(abs(small)) == tbits
            assert bool(np.signbit(x)) == bool(octant & 2) and bool(np.signbit(y)) == bool(octant & 4)
    # the last index of an octant is t = 1, the first of the next t = 0
    assert P.decode_atan2_octant(P.UNIT_FLOATS - 1) == (1, 1) and P.decode_atan2_octant(P.UNIT_FLOATS) == (1, 0)
    n = len(P.divisors())
    for j in range(n):
        for abits in [0, 1, P.BELOW_ONE - 1] + list(rng.integers(0, P.BELOW_ONE, 20)):
            jj, a = P.decode_div(P.encode_div(j, abits))
            assert jj == j and P.bits_of(a) == abits and 0 <= a < 1
    assert P.grid_point(0) == (0, 0) and P.grid_point(2048 * 4096 + 2048) == (0.5, 0.5)
    assert P.grid_point((2 << 24) + 4095 * 4096 + 1) == (f32(1 / 4096), f32(4095 / 4096))
    lo, hi = P.split_index([5, (7 << 32) | 9])
    assert list(lo.view(np.uint32)) == [5, 9] and list(hi.view(np.uint32)) == [0, 7]


# ------------------------------------------------------------------ the lists and the ranges
def test_divisors_are_what_the_docstring_says():
    d = P.divisors()
    assert d.dtype == np.float32 and len(d) == 71 and len(set(d.tolist())) == 71
    spread = d[:P.N_SPREAD_DIVISORS]
    assert len(spread) == 64 and (spread > 2.0 ** -20).all() and (spread <= 1).all() and (np.diff(spread) < 0).all()
    # at least 3 in every decade of (2^-20, 1], and no two mantissas alike
    assert np.histogram(np.log2(spread), bins=10, range=(-20, 0))[0].min() >= 3
    assert len(set(np.frexp(spread)[0].tolist())) == 64
    ends = d[64:].tolist()
    assert ends == [1.0, f32(1 - 2.0 ** -24), P.float_of(P.bits_of(2.0 ** -20) + 1), 2.0 ** -100,
                    P.float_of(P.bits_of(2.0 ** -100) - 1), 2.0 ** -126, 2.0 ** 126]
    with np.errstate(all="ignore"):
        rb = np.float32(1) / d
    # the fast path's condition |rb| <= 2^100 splits them as the docstring says; no reciprocal is subnormal
    assert (rb[:68] <= 2.0 ** 100).all() and (rb[68:70] > 2.0 ** 100).all() and rb[67] == 2.0 ** 100 and rb[70] == 2.0 ** -126


def test_edge_lists_hold_the_zeros_the_subnormal_ends_and_every_switch():
    for name in P.PRIMS:
        e = P.edges(name)
        assert e == sorted(set(e)) and all(0 <= b < 1 << 32 for b in e)
        for b in (0, P.SIGN, 1, 0x007FFFFF, 0x00800000):
            assert b in e, (name, b)
    for name, x in (("asin_half_chord", 0.7075), ("elevation_fast", 1.0), ("atan_unit", 1.0), ("sin", P.EIGHT_PI), ("erfinv_fast", P.ERFINV_MAX),
                    ("erfinv_fast", -P.ERFINV_MAX)):
        b = P.bits_of(x)
        assert b in P.edges(name) and b - 1 in P.edges(name) and P.in_domain(name, b) and not P.in_domain(name, b + 1), name
    # the switches, +-1 ulp
    for name, x in (("elevation_fast", 0.70710678), ("erfinv_fast", np.sqrt(1 - np.exp(-5.0))), ("erfinv_fast", -np.sqrt(1 - np.exp(-5.0))),
                    ("fast_exp2", -126.0), ("fast_exp2", 128.0), ("fast_rcp", 2.0 ** 126), ("log2", 1.0)):
        b = P.bits_of(x)
        assert {b - 1, b, b + 1} <= set(P.edges(name)), name
    # every quadrant boundary of the Cody-Waite reduction within 8 pi, both signs
    s = set(P.edges("sin"))
    for k in range(16):
        for sign in (1.0, -1.0):
            b = P.bits_of(sign * (k + 0.5) * np.pi / 2)
            assert {b - 1, b, b + 1} <= s
    assert (16 + 0.5) * np.pi / 2 > P.EIGHT_PI
    assert len(P.edges("sin")) == len(P.edges("cos")) >= 8 + 2 + 96 + 48 - 4
    # w = 5 at the listed switch: on the two sides of it in fp32
    b = P.bits_of(np.sqrt(1 - np.exp(-5.0)))
    w = [-np.log1p(-np.float64(P.float_of(p)) ** 2) for p in (b - 1, b + 1)]
    assert w[0] < 5 < w[1]


def test_swept_ranges_are_the_stated_domains():
    total = {n: sum(c for _, c in case.ranges) for n, case in P.CASES.items()}
    assert total["fast_rcp"] == 2 * (252 * (1 << 23) + 1)             # binades 2^-126 .. 2^125 and 2^126, both signs
    assert total["fast_sqrt"] == total["fast_rsq"] == 254 * (1 << 23)  # every positive normal
    assert total["asin_half_chord"] == P.bits_of(0.7075) + 1
    assert total["elevation_fast low"] + total["elevation_fast high"] == P.UNIT_FLOATS == total["atan_unit"]
    assert total["sincos_fast sin"] == 2 * (P.bits_of(P.EIGHT_PI) + 1)
    assert total["erfinv_fast"] == 2 * (P.bits_of(1.0) - 1) and P.float_of(P.bits_of(1.0) - 2) == P.ERFINV_MAX
    assert total["log2 low w"] + total["log2 high w"] == P.bits_of(1.0) - P.bits_of(2.0 ** -23) + 1
    assert total["fast_exp2"] == P.bits_of(128.0) + (P.bits_of(-126.0) - P.SIGN + 1)
    assert sum(c for _, c in P.ALL_PATTERNS) == 1 << 32
    for name, case in P.CASES.items():
        for first, count in case.ranges:
            assert P.in_domain(case.prim, first) and P.in_domain(case.prim, first + count - 1), name
    # the image of 2 s - 1 over [kEpsilon, kOneMinusEpsilon] in fp32
    assert f32(np.float32(2) * np.float32(1 - 2.0 ** -24) - np.float32(1)) == P.ERFINV_MAX
    assert f32(np.float32(2) * np.float32(P.K_EPSILON) - np.float32(1)) == -P.ERFINV_MAX
    # the smallest argument of the logarithm inside erfinv_fast lies in the swept range
    assert f32(1 - np.float64(P.ERFINV_MAX) ** 2) >= 2.0 ** -23
    rb = P.random_bits("sin", P.CASES["sincos_fast sin"].ranges)
    assert len(rb) == P.N_RANDOM and all(P.in_domain("sin", int(b)) for b in rb) and (rb >= P.SIGN).any() and (rb < P.SIGN).any()


def test_derived_bounds_are_the_documented_numbers():
    assert abs(P.EXP2_ULP - 8.39) < 0.005 and abs(P.ERFINV_ULP - 4.45) < 0.005 and abs(P.ERFINV_PAIR_ULP - 2.97) < 0.005
    assert abs(P.LOG2_ABS_LOW_W - 8.50e-7) < 5e-10 and abs(P.LOG2_ABS_HIGH_W - 2.32e-6) < 5e-9
    assert abs(P.CHORD_ANGLE_ULP - 7.15) < 0.005 and abs(P.ELEVATION_HIGH_ULP - 4.11) < 0.01
    assert abs(P.GAMMA_ABS - 8.8e-7) < 5e-9 and abs(P.COS_GAMMA_ABS - 6.6e-7) < 5e-9 and abs(P.DISK_ABS - 4.8e-7) < 5e-9
    assert P.SINCOS_ULP == 0.5 + 1.0 + 0.69 + 0.06 and 1.062e-7 / 2.0 ** -24 < P.SINCOS_ULP
    assert P.ATAN_UNIT_ULP == 1.4 and P.SINCOS_ABS == 1.07e-7 and abs(2 * np.sqrt(2) * P.SINCOS_ABS + 2.0 ** -23 - P.DISK_SLACK) < 1e-8
    assert P.SINCOS_ABS < P.SINCOS_CALLER_ABS and abs(P.SINCOS_CALLER_ABS - 1.67e-6) < 5e-9
    probe = open(os.path.join(ROOT, "tests", "cpp", "math_probe.hip")).read()
    assert float(re.search(r"kDiskSlack = ([0-9.e-]+);", probe).group(1)) == P.DISK_SLACK


# ------------------------------------------------------------------ what the docstrings lean on
def read_tgmm_table():
    """The SSKYPAK1 layout documented in tools/pack_datasets.py."""
    raw = open(ss.default_dataset_path(), "rb").read()
    assert raw[:8] == b"SSKYPAK1"
    _, n = struct.unpack_from("<II", raw, 8)
    for k in range(n):
        e = struct.unpack_from("<24sII6QQII", raw, 16 + 96 * k)
        if e[0].rstrip(b"\0").decode() == "tgmm_tables":
            shape = tuple(e[3:3 + e[2]])
            return np.frombuffer(raw, np.float32, int(np.prod(shape)), e[9]).reshape(shape)
    raise KeyError("tgmm_tables")


def test_tgmm_table_keeps_the_sampled_angles_inside_the_swept_domains():
    """(mu_phi, mu_theta, sigma_phi, sigma_theta, weight) per gaussian: the means lie inside the
    truncation limits [0, 2 pi] x [0, pi/2], so a truncated sample is within 2 pi of its mean (the
    erfinv bound) and the azimuth handed to sincos_fast is at most 2 pi + |sun_phi - pi/2| <= 4.5 pi,
    below 8 pi with any rounding of the cdf ends; the largest sigma is the 6.0 the docstring names."""
    t = read_tgmm_table()
    assert t.shape[-1] == 5
    assert t[..., 0].min() >= 0 and t[..., 0].max() <= f32(2 * np.pi)
    assert t[..., 1].min() >= 0 and t[..., 1].max() <= f32(np.pi / 2)
    assert t[..., 2:4].max() == 6.0 and t[..., 2:4].min() > 0
    assert 2 * np.pi + (2 * np.pi + np.pi / 2) < 8 * np.pi
    # sigma = 6 reaches the 2 pi limit at |erfinv| = 0.74
    assert abs(2 * np.pi / (np.sqrt(2) * 6.0) - 0.74) < 0.005


def test_the_pdf_mask_keeps_atan2_fast_away_from_a_subnormal_larger_component():
    """compute_pdfs masks sin_theta = sqrt(fma(x, x, y * y)) = 0: with both components below 2^-75 the
    fp32 sum of squares is 0, so the larger component of an unmasked direction is at least 2^-75,
    normal, and v_rcp of it is finite."""
    for big in (2.0 ** -126, P.float_of(P.SUBNORMAL_MAX), 2.0 ** -76, P.float_of(P.bits_of(2.0 ** -75) - 1)):
        x = np.float32(big)
        s = np.float32(np.float64(x) * np.float64(x) + np.float64(np.float32(np.float64(x) * np.float64(x))))
        assert s == 0, big
    x = np.float32(2.0 ** -74)
    assert np.float32(np.float64(x) * np.float64(x)) == np.float32(2.0 ** -148) != 0
    assert 2.0 ** -75 > 2.0 ** -126 and np.isfinite(np.float32(1) / np.float32(2.0 ** -75))


def test_values_function_numbers_are_the_kernels_cases():
    """The FN_* constants the host passes are the cases of math_probe_values' switch, no more, no fewer."""
    probe = open(os.path.join(ROOT, "tests", "cpp", "math_probe.hip")).read()
    body = probe[probe.index("void math_probe_values("):]
    assert sorted(int(n) for n in re.findall(r"^    case (\d+):", body, re.M)) == P.FN_ALL
    named = {v for k, v in vars(P).items() if k.startswith("FN_") and isinstance(v, int)}
    assert named | {P.FN_CONE_XY + 1, P.FN_CONE_XY + 2, P.FN_CONE_Z + 1, P.FN_CONE_Z + 2} == set(P.FN_ALL)
    assert {p.fn for p in P.PRIMS.values()} == set(range(10))


# ------------------------------------------------------------------ the build rule
def make_variable(text, name):
    m = re.search(r"^%s\s*[:?]?=\s*((?:.*\\\n)*.*)$" % name, text, re.M)
    assert m, name
    return " ".join(m.group(1).replace("\\\n", " ").split())


def test_probe_is_built_with_the_products_flags_and_sources():
    product = open(os.path.join(ROOT, "mitsuba3-sunsky_amd", "csrc", "Makefile")).read()
    probe = open(os.path.join(ROOT, "tests", "cpp", "Makefile")).read()
    assert make_variable(probe, "HIPFLAGS") == make_variable(product, "HIPFLAGS")
    assert make_variable(probe, "ARCH") == make_variable(product, "ARCH")
    src = make_variable(product, "KERNEL_SRC").replace("$(wildcard kernels/*.h)", "kernels/*.h").split()
    mine = make_variable(probe, "KERNEL_SRC").replace("$(wildcard $(KCSRC)/kernels/*.h)", "$(KCSRC)/kernels/*.h").split()
    assert mine == ["$(KCSRC)/" + s for s in src]
    assert "build/math_probe.hsaco: math_probe.hip $(KERNEL_SRC)" in probe
    assert re.search(r"^all:.*build/math_probe\.hsaco", probe, re.M)
    assert "$(HIPCC) $(HIPFLAGS) -I../../include -I$(KCSRC) -o $@ math_probe.hip" in probe
    first = open(os.path.join(ROOT, "tests", "cpp", "math_probe.hip")).readline()
    assert first.strip() == '#include "sunsky_kernels.hip"'
