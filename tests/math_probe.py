"""Host side of the device-math probe (tests/cpp/math_probe.hip, built by tests/cpp/Makefile into
tests/cpp/build/math_probe.hsaco): the fp32 ulp metric, an mpmath reference at 128 bits for every
primitive, the index decoders of the two-argument sweeps, the divisor and edge lists, and the
loader / launcher (hipModuleLoad through ctypes on torch-allocated buffers, as bench.py loads
clock_probe.hsaco).

The sweep kernels judge each primitive against the device's fp64 libm, which is itself code under
measurement, so confirm() re-derives every sweep's verdict here: the values kernel's fp32 results
at each block's reported worst argument, at a fixed edge list and at 4096 seeded random arguments
are compared with mpmath, and at each reported argument the device's figure has to agree with
the mpmath figure within 1e-3 ulp (double libm is ~1e-16 relative = ~1e-9 fp32 ulp: a larger gap
means the on-device reference is wrong and the sweep proves nothing).

Importing this module needs no GPU; Probe() does."""
import ctypes
import os

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HSACO = os.path.join(ROOT, "tests", "cpp", "build", "math_probe.hsaco")

MP = mpmath.mp.clone()
MP.prec = 128
ROWS = 1024                    # blocks per sweep launch = rows of its output
NONE = (1 << 64) - 1           # "no argument" in a row whose maximum is 0
AGREE_ULP = 1e-3               # device figure vs mpmath figure at a reported argument
N_RANDOM = 4096

UNIT_FLOATS = 0x3F800001       # the floats of [0, 1]
BELOW_ONE = 0x3F800000         # the floats of [0, 1)
SIGN = 0x80000000
SUBNORMAL_MIN, SUBNORMAL_MAX, NORMAL_MIN, FLOAT_MAX, INF = 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000
TWO_PI = 6.283185307179586476925
K_EPSILON = 2.0 ** -24         # sunsky_math.h kEpsilon
ERFINV_MAX = 1.0 - 2.0 ** -23  # 2 s - 1 at s = kOneMinusEpsilon; -that at s = kEpsilon
EIGHT_PI = float(np.float32(8 * np.pi))


def bits_of(x):
    return int(np.float32(x).view(np.uint32))


def float_of(b):
    return float(np.uint32(b).view(np.float32))


def floats_of(b):
    return np.asarray(b, dtype=np.uint64).astype(np.uint32).view(np.float32)


def span(lo, hi):
    """(first, count) of the bit patterns of the floats lo .. hi, both of one sign."""
    a, b = bits_of(lo), bits_of(hi)
    a, b = min(a, b), max(a, b)
    return a, b - a + 1


# ------------------------------------------------------------------ the metric
def ulp_size(ref):
    """The fp32 ulp at ref: 2^(max(floor(log2 |ref|), -126) - 23), as an mpf."""
    ref = MP.mpf(ref)
    e = -126 if ref == 0 else max(MP.frexp(ref)[1] - 1, -126)
    return MP.ldexp(MP.mpf(1), e - 23)


def errors(got, ref):
    """(ulp, abs) of the fp32 value got against ref; inf where got is not finite."""
    got = float(got)
    if not np.isfinite(got):
        return float("inf"), float("inf")
    ref = MP.mpf(ref)
    d = abs(MP.mpf(got) - ref)
    return float(d / ulp_size(ref)), float(d)


# ------------------------------------------------------------------ references (mpmath, 128 bits)
def ref_erfinv(x):
    """erfinv by Newton steps on erf from mpmath's own erfinv at 53 bits (each step squares the
    relative error: 1e-15 -> 1e-30 -> below 2^-113)."""
    x = MP.mpf(x)
    if x == 0:
        return x
    y = MP.mpf(mpmath.erfinv(float(x))) if abs(x) < 1 else MP.inf * MP.sign(x)
    if not MP.isfinite(y):
        return y
    c = MP.sqrt(MP.pi) / 2
    for _ in range(3):
        y = y - (MP.erf(y) - x) * c * MP.exp(y * y)
    return y


def ref_chord_angle(x, y, z):
    """2 asin(|v - e_z| / 2) of the vector as given (theta_upper_fast's form)."""
    x, y, dz = MP.mpf(x), MP.mpf(y), MP.mpf(z) - 1
    return 2 * MP.asin(MP.sqrt(x * x + y * y + dz * dz) / 2)


def ref_dir_terms(sn, wo, far):
    """(gamma, cos gamma) of dir_terms' form on the vectors as given; far: the sign of the fp32 dot."""
    s = -1 if far else 1
    v = [MP.mpf(float(w)) - s * MP.mpf(float(n)) for w, n in zip(wo, sn)]
    h2 = (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) / 4
    t = 2 * MP.asin(MP.sqrt(h2))
    c = 1 - 2 * h2
    return (MP.pi - t, -c) if far else (t, c)


def ref_disk(sx, sy):
    """square_to_uniform_disk_concentric."""
    x, y = 2 * MP.mpf(sx) - 1, 2 * MP.mpf(sy) - 1
    if x == 0 and y == 0:
        return MP.mpf(0), MP.mpf(0)
    q13 = abs(x) < abs(y)
    r, rp = (y, x) if q13 else (x, y)
    phi = MP.pi / 4 * rp / r
    if q13:
        phi = MP.pi / 2 - phi
    return r * MP.cos(phi), r * MP.sin(phi)


def ref_cone(sx, sy, cos_cutoff):
    """square_to_uniform_cone with the fp32 cos_cutoff as given."""
    px, py = ref_disk(sx, sy)
    cc = MP.mpf(float(cos_cutoff))
    omc, pn = 1 - cc, px * px + py * py
    sc = MP.sqrt(max(omc * (2 - omc * pn), 0))
    return px * sc, py * sc, cc + omc * (1 - pn)


def ref_atan2(y, x):
    """atan2 with IEEE signed zeros (mpmath has none): the result carries y's sign, and y = +-0 gives
    +-pi for x < 0 or x = -0."""
    y, x = float(y), float(x)
    r = (MP.pi if np.signbit(x) else MP.mpf(0)) if y == 0 else abs(MP.atan2(MP.mpf(y), MP.mpf(x)))
    return -r if np.signbit(y) else r


REF = {
    "rcp": lambda x: 1 / MP.mpf(x),
    "rsq": lambda x: 1 / MP.sqrt(MP.mpf(x)),
    "sqrt": lambda x: MP.sqrt(MP.mpf(x)),
    "exp2": lambda x: MP.power(2, MP.mpf(x)),
    "log2": lambda x: MP.log(MP.mpf(x)) / MP.ln2,
    "asin": lambda x: MP.asin(MP.mpf(x)),
    "atan": lambda x: MP.atan(MP.mpf(x)),
    "sin": lambda x: MP.sin(MP.mpf(x)),
    "cos": lambda x: MP.cos(MP.mpf(x)),
    "erfinv": ref_erfinv,
    "atan2": lambda y, x: ref_atan2(y, x),
}

# numpy / scipy fp64 counterparts, for tests/test_device_math_reference_cpu.py
def _scipy_erfinv(x):
    from scipy.special import erfinv
    return erfinv(x)


REF64 = {
    "rcp": lambda x: 1.0 / x, "rsq": lambda x: 1.0 / np.sqrt(x), "sqrt": np.sqrt, "exp2": np.exp2, "log2": np.log2,
    "asin": np.arcsin, "atan": np.arctan, "sin": np.sin, "cos": np.cos, "erfinv": _scipy_erfinv, "atan2": np.arctan2,
}
# (low, high) of the 1e4 comparison points of each
REF64_DOMAIN = {
    "rcp": (1e-30, 1e30), "rsq": (1e-30, 1e30), "sqrt": (1e-30, 1e30), "exp2": (-126.0, 127.0), "log2": (1e-38, 1e38),
    "asin": (0.0, 0.7075), "atan": (0.0, 1.0), "sin": (-25.2, 25.2), "cos": (-25.2, 25.2), "erfinv": (-0.9999998, 0.9999998),
}


# ------------------------------------------------------------------ sweeps: kernel, values function, reference
# The `fn` numbers of math_probe_values (the cases of its switch in tests/cpp/math_probe.hip;
# tests/test_device_math_reference_cpu.py holds the two sides together)
FN_RCP, FN_RSQ, FN_SQRT, FN_EXP2, FN_LOG2, FN_ASIN, FN_ELEVATION, FN_ATAN, FN_SINCOS, FN_ERFINV = range(10)
FN_WAVELENGTH, FN_DIV, FN_ATAN2 = 10, 11, 12   # (node, IEEE quotient); (div_by_rcp, IEEE quotient) of (a, b); atan2_fast(y, x)
FN_DIR_ZERO_DOT = 14                           # dir_terms<true> at a signed-zero dot: (gamma, cos gamma)
FN_DISK = 15                                   # disk_concentric_dev<true>(sx, sy): (px, py)
FN_CONE_XY = 16                                # + aperture (0, 1, 2): uniform_cone_dev<true>'s (x, y)
FN_CIRCLE_POINT = 20                           # the atan2 circle sweep's (y, x) of an index
FN_THETA_XY, FN_THETA_Z = 21, 22               # the theta sweep's (v.x, v.y), (v.z, theta_upper_fast(v)) of an index
FN_DIR_WO_XY, FN_DIR_WO_Z, FN_DIR_SUN, FN_DIR_COS = 23, 24, 25, 26   # the dir_terms sweep's (wo.x, wo.y), (wo.z, gamma), (sn.x, sn.z), (cos gamma, h)
FN_CONE_Z = 30                                 # + aperture: (z, cos_cutoff)
FN_ALL = sorted([*range(13), 14, 15, 16, 17, 18, 20, 21, 22, 23, 24, 25, 26, 30, 31, 32])


class Prim:
    def __init__(self, kernel, fn, out, ref, skip_small=False):
        self.kernel, self.fn, self.out, self.ref, self.skip_small = kernel, fn, out, ref, skip_small


# one-argument primitives: the sweep index is the argument's bit pattern
PRIMS = {
    "fast_rcp": Prim("rcp", FN_RCP, 0, REF["rcp"]),
    "fast_rsq": Prim("rsq", FN_RSQ, 0, REF["rsq"]),
    "fast_sqrt": Prim("sqrt", FN_SQRT, 0, REF["sqrt"]),
    "fast_exp2": Prim("exp2", FN_EXP2, 0, REF["exp2"]),
    "log2": Prim("log2", FN_LOG2, 0, REF["log2"]),
    "asin_half_chord": Prim("asin_half_chord", FN_ASIN, 0, REF["asin"]),
    "elevation_fast": Prim("elevation", FN_ELEVATION, 0, REF["asin"]),
    "atan_unit": Prim("atan_unit", FN_ATAN, 0, REF["atan"]),
    "sin": Prim("sin", FN_SINCOS, 0, REF["sin"]),
    "cos": Prim("cos", FN_SINCOS, 1, REF["cos"]),
    "sin_big": Prim("sin_big", FN_SINCOS, 0, REF["sin"], skip_small=True),
    "cos_big": Prim("cos_big", FN_SINCOS, 1, REF["cos"], skip_small=True),
    "erfinv_fast": Prim("erfinv_fast", FN_ERFINV, 0, REF["erfinv"]),
    "erfinv_ref": Prim("erfinv_ref", FN_ERFINV, 1, REF["erfinv"]),
}
SMALL = 1e-3   # tools/fit_sincos.py states its ulp figure for |value| > 1e-3


# ------------------------------------------------------------------ decoders of the two-argument sweeps
def encode_atan2_octant(octant, tbits):
    return int(octant) * UNIT_FLOATS + int(tbits)


def decode_atan2_octant(idx):
    """index -> (y, x): (x, y) = (1, t) with t = the float of idx % 0x3f800001; octant bit 0 swaps the
    components, bit 1 negates x, bit 2 negates y."""
    octant, tbits = divmod(int(idx), UNIT_FLOATS)
    assert 0 <= octant < 8
    x, y = np.float32(1), np.uint32(tbits).view(np.float32)
    if octant & 1:
        x, y = y, x
    if octant & 2:
        x = -x
    if octant & 4:
        y = -y
    return np.float32(y), np.float32(x)


def encode_div(j, abits):
    return int(j) * BELOW_ONE + int(abits)


def decode_div(idx):
    """index -> (divisor number, a)."""
    j, abits = divmod(int(idx), BELOW_ONE)
    return j, np.uint32(abits).view(np.float32)


def grid_point(idx):
    """index -> (sx, sy) of the 4096 x 4096 sample grid."""
    idx = int(idx) & ((1 << 24) - 1)
    return np.float32((idx & 4095) / 4096.0), np.float32((idx >> 12) / 4096.0)


def split_index(idx):
    """64-bit indices as the (low, high) words the values kernel takes in its two float inputs."""
    idx = np.asarray(idx, dtype=np.uint64)
    return (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32), (idx >> np.uint64(32)).astype(np.uint32).view(np.float32)


# div_by_rcp's divisors: 64 spread over (2^-20, 1] (w_sky, 1 - w_sky and pmf * norm magnitudes), then
# the ends of that range and the reciprocals at the limits of the fast path: b = 2^-100 (rb = 2^100,
# the largest it takes), the float below it and 2^-126 (rb above 2^100: the plain division), and
# 2^126 (rb = 2^-126, the smallest normal reciprocal)
def divisors():
    spread = [np.float32(2.0 ** (-19.7 * (k + 0.5) / 64.0)) for k in range(64)]   # 64 different mantissas
    ends = [np.float32(1), np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(2.0 ** -20), np.float32(1)),
            np.float32(2.0 ** -100), np.nextafter(np.float32(2.0 ** -100), np.float32(0)), np.float32(2.0 ** -126),
            np.float32(2.0 ** 126)]
    return np.array(spread + ends, dtype=np.float32)


N_SPREAD_DIVISORS = 64


# ------------------------------------------------------------------ edge lists
def _around(x):
    """The float x and its two neighbours (bit patterns; x of either sign, not 0)."""
    b = bits_of(x)
    return [b - 1, b, b + 1]


COMMON_EDGES = [0, SIGN, SUBNORMAL_MIN, SUBNORMAL_MAX, NORMAL_MIN, SIGN | SUBNORMAL_MIN, SIGN | SUBNORMAL_MAX, SIGN | NORMAL_MIN]


def edges(name):
    """Bit patterns: +-0, the smallest and largest subnormal, the smallest normal, then the
    primitive's domain ends with their neighbours and every branch switch +-1 ulp."""
    e = list(COMMON_EDGES)
    if name in ("fast_rcp", "fast_rsq", "fast_sqrt", "log2"):
        e += _around(1.0) + _around(2.0 ** 126) + [FLOAT_MAX, INF, SIGN | INF, 0x7FC00000] + _around(-1.0)
        e += [bits_of(2.0 ** -126) + 1, bits_of(2.0 ** 127)]
    elif name == "fast_exp2":
        e += _around(-126.0) + _around(-149.0) + _around(-150.0) + _around(128.0) + _around(127.0) + _around(1.0) + _around(-1.0)
        e += [FLOAT_MAX, INF, SIGN | INF, 0x7FC00000]
    elif name == "asin_half_chord":
        e += _around(0.7075)[:2] + _around(0.70710678) + _around(0.5)
    elif name == "elevation_fast":
        e += _around(0.70710678) + [bits_of(1.0) - 1, bits_of(1.0)] + _around(0.5)
    elif name == "atan_unit":
        e += [bits_of(1.0) - 1, bits_of(1.0)] + _around(0.5)
    elif name in ("sin", "cos", "sin_big", "cos_big"):
        # the domain ends and the quadrant boundaries of the reduction, (k + 1/2) pi/2, k = 0 .. 15
        e += [bits_of(EIGHT_PI) - 1, bits_of(EIGHT_PI)]
        for k in range(16):
            for s in (1.0, -1.0):
                e += _around(s * (k + 0.5) * np.pi / 2)
        for k in range(1, 17):   # the multiples of pi/2, where one output is smallest
            e += _around(k * np.pi / 2)
    elif name in ("erfinv_fast", "erfinv_ref"):
        # w = -log(1 - x^2) = 5 at x = sqrt(1 - e^-5)
        sw = float(np.sqrt(1 - np.exp(-5.0)))
        for s in (1.0, -1.0):
            e += _around(s * sw) + [bits_of(s * ERFINV_MAX) - 1, bits_of(s * ERFINV_MAX)] + _around(s * 0.5)
    return sorted(set(int(b) for b in e))


def in_domain(name, b):
    """Whether the bit pattern lies in the domain the bound is asserted on."""
    x = float_of(b)
    if not np.isfinite(x):
        return False
    if name in ("fast_rcp",):
        return 2.0 ** -126 <= abs(x) <= 2.0 ** 126
    if name in ("fast_rsq", "fast_sqrt", "log2"):
        return 2.0 ** -126 <= x
    if name == "fast_exp2":
        return -126.0 <= x < 128.0
    if name == "asin_half_chord":
        return 0.0 <= x <= float(np.float32(0.7075)) and not (b & SIGN)
    if name in ("elevation_fast", "atan_unit"):
        return 0.0 <= x <= 1.0 and not (b & SIGN)
    if name in ("sin", "cos", "sin_big", "cos_big"):
        return abs(x) <= EIGHT_PI
    if name in ("erfinv_fast", "erfinv_ref"):
        return abs(x) <= ERFINV_MAX
    raise KeyError(name)


def random_bits(name, ranges, seed=0):
    """N_RANDOM seeded bit patterns, uniform over the swept (first, count) ranges."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    counts = np.array([c for _, c in ranges], dtype=np.float64)
    which = rng.choice(len(ranges), N_RANDOM, p=counts / counts.sum())
    off = (rng.random(N_RANDOM) * counts[which]).astype(np.uint64)
    return np.array([ranges[w][0] for w in which], dtype=np.uint64) + off


# ------------------------------------------------------------------ the loader / launcher
class Sweep:
    """The rows of one or more sweep launches of one kernel and their reduction."""
    def __init__(self, rows):
        rows = np.concatenate(rows, axis=0)
        self.ulp, self.abs = rows[:, 0].copy().view(np.float64), rows[:, 2].copy().view(np.float64)
        self.ulp_arg, self.abs_arg = rows[:, 1], rows[:, 3]
        self.bad, self.visited = int(rows[:, 4].sum()), int(rows[:, 5].sum())
        i, j = int(self.ulp.argmax()), int(self.abs.argmax())
        self.max_ulp, self.max_ulp_arg = float(self.ulp[i]), int(self.ulp_arg[i])
        self.max_abs, self.max_abs_arg = float(self.abs[j]), int(self.abs_arg[j])

    def reported(self):
        """[(argument, device ulp or None, device abs or None)] of every row's worst arguments."""
        out = {}
        for a, v in zip(self.ulp_arg, self.ulp):
            if int(a) != NONE:
                out.setdefault(int(a), [None, None])[0] = float(v)
        for a, v in zip(self.abs_arg, self.abs):
            if int(a) != NONE:
                out.setdefault(int(a), [None, None])[1] = float(v)
        return [(a, u, d) for a, (u, d) in sorted(out.items())]

    def line(self):
        return (f"points {self.visited} | max ulp {self.max_ulp:.4f} at {self.max_ulp_arg:#x} | "
                f"max abs {self.max_abs:.4e} at {self.max_abs_arg:#x} | bad {self.bad}")


class Probe:
    def __init__(self, path=HSACO):
        import torch
        self.torch = torch
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")   # the HIP context, before the module is loaded
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build() (make -C tests/cpp) makes it")
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.mod = ctypes.c_void_p()
        rc = self.hip.hipModuleLoad(ctypes.byref(self.mod), path.encode())
        if rc != 0:
            raise RuntimeError(f"hipModuleLoad({path}) -> {rc}")
        self._fns = {}

    def close(self):
        if self.mod:
            self.torch.cuda.synchronize()
            self.hip.hipModuleUnload(self.mod)
            self.mod = ctypes.c_void_p()

    def _function(self, name):
        if name not in self._fns:
            fn = ctypes.c_void_p()
            rc = self.hip.hipModuleGetFunction(ctypes.byref(fn), self.mod, name.encode())
            if rc != 0:
                raise RuntimeError(f"hipModuleGetFunction({name}) -> {rc}")   # a missing kernel is an error
            self._fns[name] = fn
        return self._fns[name]

    def _launch(self, name, blocks, args):
        stream = self.torch.cuda.current_stream().cuda_stream
        argv = (ctypes.c_void_p * len(args))(*[ctypes.cast(ctypes.pointer(a), ctypes.c_void_p) for a in args])
        rc = self.hip.hipModuleLaunchKernel(self._function(name), ctypes.c_uint(blocks), ctypes.c_uint(1), ctypes.c_uint(1),
                                            ctypes.c_uint(256), ctypes.c_uint(1), ctypes.c_uint(1), ctypes.c_uint(0),
                                            ctypes.c_void_p(stream), argv, None)
        if rc != 0:
            raise RuntimeError(f"hipModuleLaunchKernel({name}) -> {rc}")
        self.torch.cuda.synchronize()

    def sweep(self, kernel, ranges, aux=None):
        """Run math_probe_sweep_<kernel> over each (first, count) of ranges."""
        torch = self.torch
        aux_t = torch.zeros(1, dtype=torch.float32, device="cuda") if aux is None else \
            torch.from_numpy(np.ascontiguousarray(aux, dtype=np.float32)).cuda()
        aux_n = 0 if aux is None else aux_t.numel()
        rows = []
        for first, count in ranges:
            out = torch.full((ROWS, 6), -1, dtype=torch.int64, device="cuda")
            self._launch("math_probe_sweep_" + kernel, ROWS,
                         [ctypes.c_uint64(int(first)), ctypes.c_uint64(int(count)), ctypes.c_uint64(ROWS),
                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(aux_t.data_ptr()), ctypes.c_uint64(aux_n)])
            r = out.cpu().numpy().view(np.uint64)
            assert (r[:, 5] != NONE).all(), "a block wrote no row"
            assert int(r[:, 5].sum()) == int(count), "the sweep did not visit every argument"
            rows.append(r)
        return Sweep(rows)

    def values(self, fn, x, y=None):
        """(out0, out1) of math_probe_values for the fp32 lists x (and y)."""
        torch = self.torch
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, dtype=np.float32)
        assert x.shape == y.shape and x.ndim == 1
        n = x.size
        if n == 0:
            return np.zeros(0, np.float32), np.zeros(0, np.float32)
        # bit patterns travel as they are (NaN payloads, signed zeros): integer tensors, viewed as float on the device
        xt = torch.from_numpy(x.view(np.int32).copy()).cuda()
        yt = torch.from_numpy(y.view(np.int32).copy()).cuda()
        o0 = torch.zeros(n, dtype=torch.int32, device="cuda")
        o1 = torch.zeros(n, dtype=torch.int32, device="cuda")
        self._launch("math_probe_values", (n + 255) // 256,
                     [ctypes.c_int(fn), ctypes.c_void_p(xt.data_ptr()), ctypes.c_void_p(yt.data_ptr()),
                      ctypes.c_void_p(o0.data_ptr()), ctypes.c_void_p(o1.data_ptr()), ctypes.c_uint64(n)])
        return o0.cpu().numpy().view(np.float32), o1.cpu().numpy().view(np.float32)


# ------------------------------------------------------------------ the host's re-derivation
class Confirmed:
    """Host maxima (mpmath) over the reported, edge and random arguments that lie in the domain."""
    def __init__(self):
        self.max_ulp = self.max_abs = 0.0
        self.max_ulp_arg = self.max_abs_arg = None
        self.checked = 0

    def add(self, arg, ulp, ab):
        self.checked += 1
        if ulp > self.max_ulp:
            self.max_ulp, self.max_ulp_arg = ulp, arg
        if ab > self.max_abs:
            self.max_abs, self.max_abs_arg = ab, arg


def _agree(name, arg, dev_ulp, dev_abs, ulp, ab, ref):
    if dev_ulp is not None:
        assert abs(dev_ulp - ulp) <= AGREE_ULP, f"{name} at {arg:#x}: device {dev_ulp} ulp, mpmath {ulp} ulp"
    if dev_abs is not None:
        assert abs(dev_abs - ab) <= AGREE_ULP * float(ulp_size(ref)), f"{name} at {arg:#x}: device abs {dev_abs}, mpmath {ab}"


def confirm(probe, name, sweep, ranges):
    """One-argument primitive: see the module docstring.  Returns the host's maxima; asserts the
    device's figures at its reported arguments, and that no in-domain edge or random argument
    exceeds the sweep's maxima."""
    prim = PRIMS[name]
    rep = sweep.reported()
    extra = [b for b in edges(name) if in_domain(name, b) and any(f <= b < f + c for f, c in ranges)]
    extra += [int(b) for b in random_bits(name, ranges)]
    args = [a for a, _, _ in rep] + extra
    got = probe.values(prim.fn, floats_of(args))[prim.out]
    c = Confirmed()
    for k, (arg, g) in enumerate(zip(args, got)):
        ref = prim.ref(float_of(arg))
        if prim.skip_small and abs(ref) <= SMALL:
            continue
        ulp, ab = errors(g, ref)
        if k < len(rep):
            _agree(name, arg, rep[k][1], rep[k][2], ulp, ab, ref)
        else:
            assert ulp <= sweep.max_ulp + AGREE_ULP and ab <= sweep.max_abs * (1 + 1e-6) + 1e-300, \
                f"{name} at {arg:#x}: {ulp} ulp, {ab} abs on the host exceeds the sweep's maxima {sweep.line()}"
        c.add(arg, ulp, ab)
    return c


def confirm_pairs(name, rep, pairs, got, ref_fn, sweep):
    """Two-argument primitive whose arguments the caller decoded: pairs[k] the arguments of the
    k-th entry (the first len(rep) are the sweep's reported ones), got[k] the device's fp32 result."""
    c = Confirmed()
    for k, (p, g) in enumerate(zip(pairs, got)):
        ref = ref_fn(*[float(v) for v in p])
        ulp, ab = errors(g, ref)
        if k < len(rep):
            _agree(name, rep[k][0], rep[k][1], rep[k][2], ulp, ab, ref)
        else:
            assert ulp <= sweep.max_ulp + AGREE_ULP, f"{name} at {p}: {ulp} ulp on the host exceeds the sweep's {sweep.max_ulp}"
        c.add(p, ulp, ab)
    return c


# ------------------------------------------------------------------ the swept domains and their bounds
def signed(lo, hi):
    """The ranges of +[lo, hi] and -[lo, hi]."""
    f, c = span(lo, hi)
    return [(f, c), (f | SIGN, c)]


ALL_PATTERNS = [(0, 1 << 31), (1 << 31, 1 << 31)]
F_EXP_M5 = float(np.float32(np.exp(-5.0)))
SWITCH_Z = float(np.float32(0.70710678))
PARITY_BAR = 1e-5
ULP_REL = 2.0 ** -23   # one fp32 ulp is at most this relative to the value

# The derived bounds (the derivations are in the docstrings of tests/test_gpu_device_math.py)
EXP2_ULP = PARITY_BAR / 5 / 2 / ULP_REL                  # 8.39
ERFINV_ULP = PARITY_BAR / 3 / TWO_PI / ULP_REL           # 4.45
ERFINV_SHARE = PARITY_BAR / 3 / TWO_PI / 3               # 1.77e-7 relative: log2, sqrt, polynomial
LOG2_ABS_LOW_W = ERFINV_SHARE / (0.3 * np.log(2.0))      # 8.50e-7, arguments in [e^-5, 1]
LOG2_ABS_HIGH_W = ERFINV_SHARE / (0.11 * np.log(2.0))    # 2.32e-6, arguments in [2^-23, e^-5)
ERFINV_PAIR_ULP = 2 * ERFINV_SHARE / ULP_REL             # 2.97
CHORD_ANGLE_ULP = (4.5 * 1.2733 + 2 * 0.71)              # 7.15: theta_upper_fast, dir_terms' near side
ELEVATION_HIGH_ABS = 2 * (0.392700 * 1.055 * ULP_REL + 0.71 * 2.0 ** -25) + 2.0 ** -24 + 4.38e-8   # 2.45e-7
ELEVATION_HIGH_ULP = ELEVATION_HIGH_ABS / 2.0 ** -24     # 4.11, results in [pi/4, pi/2]
GAMMA_ABS = CHORD_ANGLE_ULP * 2.0 ** -24 * (np.pi / 2) + 2.0 ** -23 + 8.75e-8   # 8.76e-7
COS_GAMMA_ABS = 11 * 2.0 ** -24                          # 6.56e-7
ATAN_UNIT_ULP = 1.4                                       # 1.4: atan2_fast's stated 4.4 ulp less the 3 ulp t = min * rcp(max) can carry
SINCOS_ABS = 1.07e-7                                      # the cosine path's operation count, tests/test_gpu_device_math.py
SINCOS_ULP = 2.25                                         # where |value| > 1e-3: the sine path's relative operation count
SINCOS_CALLER_ABS = PARITY_BAR / 3 / 2                    # 1.67e-6: what sample_sky's direction allows
DISK_ABS = (4.5 * 2.0 ** -24 * np.pi / 4 + 2.0 ** -24 + 4.38e-8) + SINCOS_ABS + 2.0 ** -24   # 4.8e-7
DISK_SLACK = 4.3e-7                                       # 2 sqrt(2) SINCOS_ABS + 2^-23 on px^2 + py^2 (kDiskSlack in the probe)


class Case:
    def __init__(self, name, prim, domain, ranges, ulp=None, ab=None, source=""):
        self.name, self.prim, self.domain, self.ranges, self.ulp, self.ab, self.source = name, prim, domain, ranges, ulp, ab, source


CASES = {c.name: c for c in [
    Case("fast_rcp", "fast_rcp", "2^-126 <= |x| <= 2^126", signed(2.0 ** -126, 2.0 ** 126), ulp=1.0, source="stated (v_rcp_f32)"),
    Case("fast_rsq", "fast_rsq", "x >= 2^-126", [span(2.0 ** -126, float_of(FLOAT_MAX))], ulp=1.0, source="stated (v_rsq_f32)"),
    Case("fast_sqrt", "fast_sqrt", "x >= 2^-126", [span(2.0 ** -126, float_of(FLOAT_MAX))], ulp=1.0, source="stated (v_sqrt_f32)"),
    Case("fast_exp2", "fast_exp2", "-126 <= x < 128", [(0, bits_of(128.0)), span(-0.0, -126.0)], ulp=EXP2_ULP, source="derived"),
    Case("log2 low w", "log2", "e^-5 <= x <= 1", [span(F_EXP_M5, 1.0)], ab=LOG2_ABS_LOW_W, source="derived"),
    Case("log2 high w", "log2", "2^-23 <= x < e^-5", [(bits_of(2.0 ** -23), bits_of(F_EXP_M5) - bits_of(2.0 ** -23))], ab=LOG2_ABS_HIGH_W,
         source="derived"),
    Case("asin_half_chord", "asin_half_chord", "0 <= x <= 0.7075", [span(0.0, 0.7075)], ulp=0.71, source="stated"),
    Case("elevation_fast low", "elevation_fast", "0 <= z <= 0.70710678", [span(0.0, SWITCH_Z)], ulp=0.71, source="stated"),
    Case("elevation_fast high", "elevation_fast", "0.70710678 < z <= 1", [(bits_of(SWITCH_Z) + 1, bits_of(1.0) - bits_of(SWITCH_Z))],
         ulp=ELEVATION_HIGH_ULP, ab=ELEVATION_HIGH_ABS, source="derived"),
    Case("atan_unit", "atan_unit", "0 <= t <= 1", [span(0.0, 1.0)], ulp=ATAN_UNIT_ULP, source="derived; stated 1.07"),
    Case("sincos_fast sin", "sin", "|x| <= 8 pi", signed(0.0, EIGHT_PI), ab=SINCOS_ABS, source="derived; stated 9.2e-8"),
    Case("sincos_fast cos", "cos", "|x| <= 8 pi", signed(0.0, EIGHT_PI), ab=SINCOS_ABS, source="derived; stated 9.2e-8"),
    Case("sincos_fast sin, |sin| > 1e-3", "sin_big", "|x| <= 8 pi", signed(0.0, EIGHT_PI), ulp=SINCOS_ULP, source="derived; stated 1.5"),
    Case("sincos_fast cos, |cos| > 1e-3", "cos_big", "|x| <= 8 pi", signed(0.0, EIGHT_PI), ulp=SINCOS_ULP, source="derived; stated 1.5"),
    Case("erfinv_fast", "erfinv_fast", "|x| <= 1 - 2^-23", signed(0.0, ERFINV_MAX), ulp=ERFINV_ULP, source="derived"),
    Case("erfinvf_", "erfinv_ref", "|x| <= 1 - 2^-23", signed(0.0, ERFINV_MAX), ulp=ERFINV_ULP, source="derived"),
]}
