"""Figures behind tests/test_gpu_device_math.py and DESIGN.md section 6 "Device math primitives"
(measured only, nothing asserted): one line per primitive of csrc/sunsky_kernels.hip's FAST math
with its swept domain, the points visited, the worst error in fp32 ulp and its argument, the worst
absolute error and its argument (both against the device's fp64 libm, tests/cpp/math_probe.hip),
the stated or derived bound and measured / bound.  Then the census of the hardware wrappers over
all 2^32 patterns, and sincos_fast past 8 pi.  Arguments are fp32 bit patterns, or the index that
tests/math_probe.py decodes for the two-argument sweeps.
usage: python tools/device_math_measure.py > profiles/device_math_measure.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("mitsuba3-sunsky_amd", "tests")]
import numpy as np  # noqa: E402
import math_probe as P  # noqa: E402

probe = P.Probe()


def line(name, domain, s, ulp=None, ab=None, source=""):
    bound = " and ".join(b for b in (f"{ulp:.4g} ulp" if ulp is not None else "", f"{ab:.4g} abs" if ab is not None else "") if b) or "-"
    ratios = [r for r in ((s.max_ulp / ulp) if ulp else None, (s.max_abs / ab) if ab else None) if r is not None]
    ratio = f"{max(ratios):.3f}" if ratios else "-"
    print(f"{name} | {domain} | {s.visited} | {s.max_ulp:.4f} at {s.max_ulp_arg:#x} | {s.max_abs:.4e} at {s.max_abs_arg:#x} | "
          f"{s.bad} | {bound} ({source}) | {ratio}", flush=True)


print("== 1. each primitive over its domain")
print("primitive | domain | points | max ulp at argument | max abs at argument | non-finite or out of range | bound | measured / bound")
for case in P.CASES.values():
    line(case.name, case.domain, probe.sweep(P.PRIMS[case.prim].kernel, case.ranges), case.ulp, case.ab, case.source)
erf_ranges = P.CASES["erfinv_fast"].ranges
line("erfinv_fast vs erfinvf_", "|x| <= 1 - 2^-23", probe.sweep("erfinv_pair", erf_ranges), P.ERFINV_PAIR_ULP, None, "derived")
line("erfinv_fast oddness (mismatches as 1)", "0 <= x <= 1 - 2^-23", probe.sweep("erfinv_odd", erf_ranges[:1]), None, None, "bit-equal")
line("sincos_fast parity (mismatches as 1)", "0 <= x <= 8 pi", probe.sweep("sincos_parity", [P.span(0.0, P.EIGHT_PI)]), None, None, "bit-equal")
line("atan2_fast octants", "(1, t), t in [0, 1], 8 octants", probe.sweep("atan2_octant", [(0, 8 * P.UNIT_FLOATS)]), 4.4, 3.5e-7, "stated")
line("atan2_fast circles", "2^24 angles x 2^(0, -4 .. -60)", probe.sweep("atan2_circle", [(0, 16 << 24)]), 4.4, 3.5e-7, "stated")
line("theta_upper_fast", "2^24 directions + 2 x 256 rings", probe.sweep("theta_upper", [(0, (1 << 24) + (2 << 20))]), P.CHORD_ANGLE_ULP, None, "derived")
line("dir_terms gamma", "3 suns x (2^20 directions + 256 rings)", probe.sweep("dir_gamma", [(0, 3 << 21)]), None, P.GAMMA_ABS, "derived")
line("dir_terms gamma, near rings", "gamma in [1e-6, 4.65e-3]",
     probe.sweep("dir_gamma", [((k << 21) + (1 << 20), 1 << 19) for k in range(3)]), P.CHORD_ANGLE_ULP, None, "derived")
line("dir_terms cos gamma", "3 suns x (2^20 directions + 256 rings)", probe.sweep("dir_cos_gamma", [(0, 3 << 21)]), None, P.COS_GAMMA_ABS, "derived")
line("disk_concentric_dev (error in 2^-24)", "4096 x 4096 grid", probe.sweep("disk_concentric", [(0, 1 << 24)]), None, P.DISK_ABS, "derived")
for k, name in enumerate(("0.2665", "5", "30")):
    line(f"uniform_cone_dev {name} deg (error in 2^-24)", "4096 x 4096 grid", probe.sweep("uniform_cone", [(k << 24, 1 << 24)]), None, P.DISK_ABS, "derived")
div = P.divisors()
line("div_by_rcp (mismatches as 1)", f"a in [0, 1) x {len(div)} divisors",
     probe.sweep("div_by_rcp", [(0, len(div) * P.BELOW_ONE)], aux=div), None, None, "bit-equal")
line("wavelength_node (mismatches as 1)", "all 2^32", probe.sweep("wavelength_node", P.ALL_PATTERNS), None, None, "bit-equal")

print("== 2. the hardware wrappers over all 2^32 patterns (errors where result and reference are finite) and at the edges")
for name in ("fast_rcp", "fast_rsq", "fast_sqrt", "fast_exp2", "log2"):
    prim = P.PRIMS[name]
    line(name, "all 2^32", probe.sweep(prim.kernel, P.ALL_PATTERNS))
    e = P.edges(name)
    for b, g in zip(e, probe.values(prim.fn, P.floats_of(e))[prim.out]):
        print(f"  {name}({P.float_of(b)!r} [{b:#010x}]) = {float(g)!r} [{P.bits_of(g):#010x}]")

print("== 3. sincos_fast past 8 pi: the worst absolute error per interval (the bound is 9.2e-8)")
lo = P.EIGHT_PI
for hi in [float(np.float32(k * np.pi)) for k in range(9, 17)] + [float(np.float32(2.0 ** k * np.pi)) for k in range(5, 12)]:
    first, count = P.span(lo, hi)
    for prim in ("sin", "cos"):
        line(f"sincos_fast {prim}", f"({lo / np.pi:.0f} pi, {hi / np.pi:.0f} pi]", probe.sweep(prim, [(first + 1, count - 1)]), None, 9.2e-8, "stated to 8 pi")
    lo = hi
probe.close()
