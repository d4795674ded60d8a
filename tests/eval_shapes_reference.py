"""Inputs, masks, sizes and the bake reference of the eval / bake call-shape tests
(tests/test_eval_shapes_cpu.py, tests/test_gpu_eval_shapes.py and its worker
tests/gpu_eval_worker.py, tools/eval_shapes_measure.py).  Numpy and the oracle only.

The bake reference restates the contract of sunsky_bake_latlong (include/sunsky_amd.h, check_bake):

    d_theta = (theta1 - theta0) / (h - 1)  in fp32 (0 for h == 1), d_phi likewise from w
    theta_y = fma(y, d_theta, theta0),  phi_x = fma(x, d_phi, phi0)      one rounding each
    d = (cos phi sin theta, sin phi sin theta, cos theta)               sin, cos rounded to fp32,
                                                                        the products formed in fp32
    pixel (x, y) = eval(wi = -d)

with the fma taken in rational arithmetic and rounded once (fma_f32), sin and cos in fp64.  The two
oracles at those directions are o32 and o64; a bake is held per pixel and channel to

    |bake - o64| <= 1e-5 max(|o64|, 1e-6 max |o64|) + |o32 - o64| + S

where S is the first-order effect of the device's direction rounding: per component c of d the
larger of |o64(d +- E_c ulp(d_c) e_c) - o64(d)|, summed over the three components.  E = (9, 9, 4):
ROCm's device sincosf is written to OpenCL's full-profile bound of 4 ulp (the OpenCL C
specification's table of relative errors: sin, cos, sincos <= 4 ulp; the installed ROCm tree ships
no document that states another bound for sincosf), z is one such value, and x, y are a
product of two such values plus the product's own rounding: (1 + 4 u)^2 (1 + u / 2) - 1 < 8.5 u,
rounded up to 9.  A pixel whose bound exceeds 1e-3 relative is "loose" (a limb pixel, where a
perturbation flips the disc mask) and proves nothing: the tests cap their number."""
import math
from fractions import Fraction

import numpy as np

import oracle as O
from helpers import angles_dict, fp32_sun_input, sphere_wo

SIZES = (1, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4099)
FRAMES = ("identity", "rotated")
COMBOS = [(v, p, f) for v in ("rgb", "spectral") for p in ("fast", "reference") for f in FRAMES]
NODES = [float(x) for x in range(320, 721, 40)]     # the 11 model wavelengths: the node kernel
OFF_NODES = [350.0, 412.5, 555.0, 633.25, 700.0]    # the general broadcast kernel
BAKE_OFF_NODES = [350.0, 300.0, 555.0, 719.99, 800.0]   # planes 1 and 4 are outside the model: exactly 0
# 32 broadcast wavelengths: duplicates, nodes, the upper edge and its neighbour, both sides outside
LIST32 = [555.0, 555.0, 320.0, 720.0, 719.99, 300.0, 800.0, 360.0, 320.01, 400.0, 440.0, 412.5, 480.0, 520.0, 633.25,
          560.0, 600.0, 640.0, 680.0, 700.0, 350.0, 350.0, 719.99, 321.0, 450.5, 500.0, 510.0, 590.0, 610.0, 650.0,
          690.0, 720.0]
EDGE_LAMBDA = np.array([320.0, 360.0, 720.0, 719.99, 320.01, 555.0, 300.0, 800.0], np.float32)
MAX_LAMBDA, MAX_BROADCAST = 16, 32                  # kMaxLambdaPerRay, kMaxBroadcastLambda
MASKS = ("none", "all_on", "all_off", "third_off", "tail_off", "body_off", "on_bytes")
ON_BYTES = np.array([1, 2, 0x80, 0xFF], np.uint8)
E_ULP = (9, 9, 4)
LOOSE = 1e-3
SUN_THETA, SUN_PHI = math.radians(50.0), 0.3

# (width, height) over the whole sphere, and the two windows
SPHERE_SIZES = [(1, 1), (1, 5), (5, 1), (2, 3), (3, 2), (4, 3), (7, 5), (8, 5), (9, 7), (37, 13), (64, 33)]
WINDOW = dict(size=(33, 17), theta=(0.2, 1.7), phi=(-1.0, 2.5))
WINDOW_REVERSED = dict(size=(33, 17), theta=(1.7, 0.2), phi=(2.5, -1.0))
SUN_WINDOW_SIZES = [(33, 33), (36, 33)]             # the scalar-store and the 16-byte-store path
LAYOUT_SIZES = [(8, 5), (9, 7), (36, 33)]


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], dtype=np.float32)


def emitter_dict(frame="identity"):
    """T = 4, the sun at phi 0.3 and theta 50 degrees, albedo 0.2; rotated: to_world a rotation of
    0.5 rad about x, which maps rows below the image's horizon back up."""
    d = angles_dict(4.0, SUN_PHI, SUN_THETA, 0.2, 1.0, 1.0)
    if frame == "rotated":
        d["to_world"] = rot_x(0.5)
    elif frame != "identity":
        raise ValueError(frame)
    return d


_ORACLES = {}


def oracles(variant, frame, d=None):
    """(o32, o64) of emitter_dict(frame) (or of d, uncached); the fp64 oracle is given the fp32
    sun direction the fp32 implementations compute (helpers.fp32_sun_input)."""
    if d is not None:
        o32 = O.Oracle(d, variant, "jit", "f32")
        return o32, O.Oracle(fp32_sun_input(d, o32), variant, "jit", "f64")
    key = (variant, frame)
    if key not in _ORACLES:
        _ORACLES[key] = oracles(variant, frame, emitter_dict(frame))
    return _ORACLES[key]


def to_world3(frame):
    return np.asarray(emitter_dict(frame).get("to_world", np.eye(4)), np.float64)[:3, :3]


def to_local(frame, wo):
    """World directions (n, 3) in the emitter's frame, fp32 (the sun-lane mask of assert_parity)."""
    return (np.asarray(wo, np.float64) @ np.linalg.inv(to_world3(frame)).T).astype(np.float32)


def sun_world(frame):
    return oracles("rgb", frame)[0].info()["sun_dir_world"]


def sun_lanes(frame, wo):
    inf = oracles("rgb", frame)[0].info()
    loc = to_local(frame, wo)
    return (loc @ inf["sun_dir_local"] >= inf["cos_cutoff"]) & (loc[:, 2] >= 0)


def _cone(n, s, g_lo, g_hi, rng):
    """n unit vectors at angles in [g_lo, g_hi] from s, fp32."""
    s = np.asarray(s, np.float64) / np.linalg.norm(s)
    a = np.array([1.0, 0, 0]) if abs(s[0]) < 0.9 else np.array([0, 1.0, 0])
    t1 = np.cross(s, a)
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(s, t1)
    g = g_lo + (g_hi - g_lo) * np.sqrt(rng.random(n))
    ph = 2 * np.pi * rng.random(n)
    return (np.cos(g)[:, None] * s + np.sin(g)[:, None] * (np.cos(ph)[:, None] * t1 + np.sin(ph)[:, None] * t2)).astype(np.float32)


def directions(n, frame, seed=101):
    """(n, 3) world directions wo: every eighth (0, 8, ...) inside the sun disc (within 0.2 degrees;
    the half aperture is 0.268), 1, 9, ... in a band of +-5 % around the limb, 2, 10, ... below the
    emitter's horizon, the rest uniform on the sphere."""
    rng = np.random.default_rng(seed)
    wo = sphere_wo(n, seed=seed + 1)
    s = sun_world(frame)
    half = np.deg2rad(0.5358 / 2)
    k = len(wo[::8])
    wo[::8] = _cone(k, s, 0.0, np.deg2rad(0.2), rng)
    k = len(wo[1::8])
    if k:
        wo[1::8] = _cone(k, s, 0.95 * half, 1.05 * half, rng)
    k = len(wo[2::8])
    if k:
        low = sphere_wo(k, seed=seed + 2).astype(np.float64)
        low[:, 2] = -np.maximum(np.abs(low[:, 2]), 1e-3)
        low /= np.linalg.norm(low, axis=1, keepdims=True)
        wo[2::8] = (low @ to_world3(frame).T).astype(np.float32)
    return wo


def lambdas(n, seed=103):
    """(16, n) per-ray wavelength planes in [320, 720], the first columns nodes, 719.99, 320.01 and
    values outside the model's range (row k rolled by k, so the rows differ)."""
    lam = np.random.default_rng(seed).uniform(320.0, 720.0, (MAX_LAMBDA, n)).astype(np.float32)
    k = min(n, EDGE_LAMBDA.size)
    for r in range(MAX_LAMBDA):
        lam[r, :k] = np.roll(EDGE_LAMBDA, r)[:k]
    return lam


def inputs(n, frame, seed=101):
    """numpy from a fixed seed: wo (3, n) world directions (directions()), lam (16, n)."""
    return dict(wo=np.ascontiguousarray(directions(n, frame, seed).T), lam=lambdas(n, seed + 2))


def mask(kind, n, seed=5):
    """The C ABI's mask plane (uint8, any non-zero byte is on), or None."""
    if kind == "none":
        return None
    m = np.ones(n, np.uint8)
    if kind == "all_off":
        m[:] = 0
    elif kind == "third_off":
        m[::3] = 0
    elif kind == "tail_off":
        m[n - n % 4:] = 0
    elif kind == "body_off":
        m[:n - n % 4] = 0
    elif kind == "on_bytes":
        rng = np.random.default_rng(seed)
        m = np.where(rng.random(n) < 0.3, 0, ON_BYTES[rng.integers(0, 4, n)]).astype(np.uint8)
        m[:min(n, 4)] = ON_BYTES[:min(n, 4)]
    elif kind != "all_on":
        raise ValueError(kind)
    return m


SPECIAL_DIRS = {"zero": (0.0, 0.0, 0.0), "nan": (np.nan, np.nan, np.nan), "nan_x": (np.nan, 0.6, 0.8),
                "inf": (np.inf, 0.0, 0.0), "minus_inf": (0.0, 0.0, -np.inf)}


def oracle_eval(o, wo, lam=None):
    """The oracle at wi = -wo (n, 3) -> (C, n): RGB, or spectral at the wavelength list lam
    (broadcast to every direction) or at the (k, n) planes lam."""
    wi = -np.asarray(wo, np.float32)
    if not o.spectral:
        return np.asarray(o.eval(wi), np.float64).T
    lam = np.asarray(lam, np.float32)
    if lam.ndim == 1:
        lam = np.repeat(lam[:, None], wi.shape[0], 1)
    return np.asarray(o.eval(wi, lam), np.float64)


# ---------------------------------------------------------------- the bake reference
def round_f32(fr):
    """The fp32 nearest to the rational fr, ties to even."""
    c = np.float32(float(fr))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(v.view(np.uint32)) & 1))


def fma_f32(a, b, c):
    """fmaf(a, b, c) for fp32 scalars: the exact a b + c rounded once."""
    return round_f32(Fraction(float(np.float32(a))) * Fraction(float(np.float32(b))) + Fraction(float(np.float32(c))))


def bake_angles(count, a0, a1):
    """The `count` angles of one axis of the image, fp32: fma(i, (a1 - a0) / (count - 1), a0)."""
    a0, a1 = np.float32(a0), np.float32(a1)
    step = np.float32((a1 - a0) / np.float32(count - 1)) if count > 1 else np.float32(0)
    return np.array([fma_f32(np.float32(i), step, a0) for i in range(count)], np.float32)


def bake_directions(w, h, theta=(0.0, math.pi), phi=(0.0, 2 * math.pi)):
    """-> (d (h w, 3) fp32 with pixel (x, y) at row y w + x, theta (h,), phi (w,))."""
    th, ph = bake_angles(h, *theta), bake_angles(w, *phi)
    st, ct = np.sin(th.astype(np.float64)).astype(np.float32), np.cos(th.astype(np.float64)).astype(np.float32)
    sp, cp = np.sin(ph.astype(np.float64)).astype(np.float32), np.cos(ph.astype(np.float64)).astype(np.float32)
    d = np.stack([(cp[None, :] * st[:, None]).astype(np.float32), (sp[None, :] * st[:, None]).astype(np.float32),
                  np.broadcast_to(ct[:, None], (h, w))], -1).reshape(-1, 3)
    return np.ascontiguousarray(d, np.float32), th, ph


def sun_window(frame, half_theta=0.01, half_phi=0.012):
    """(theta range, phi range) of the window around the sun's world direction."""
    s = sun_world(frame)
    t, p = math.acos(s[2] / np.linalg.norm(s)), math.atan2(s[1], s[0])
    return (t - half_theta, t + half_theta), (p - half_phi, p + half_phi)


class BakeReference:
    """o32, o64 (C, h w) and the bound of one image; lam: None (RGB) or the wavelength list."""

    def __init__(self, variant, frame, w, h, theta=(0.0, math.pi), phi=(0.0, 2 * math.pi), lam=None, d=None):
        o32, o64 = oracles(variant, frame, d)
        self.w, self.h = w, h
        self.d, self.theta, self.phi = bake_directions(w, h, theta, phi)
        self.o32 = oracle_eval(o32, self.d, lam)
        self.o64 = oracle_eval(o64, self.d, lam)
        s = np.zeros_like(self.o64)
        pert_zero = np.ones(self.o64.shape[1], bool)
        for c in range(3):
            step = (E_ULP[c] * np.spacing(np.abs(self.d[:, c]))).astype(np.float32)
            worst = np.zeros_like(self.o64)
            for sg in (1.0, -1.0):
                dp = self.d.copy()
                dp[:, c] = self.d[:, c] + np.float32(sg) * step
                v = oracle_eval(o64, dp, lam)
                worst = np.maximum(worst, np.abs(v - self.o64))
                pert_zero &= ~v.any(axis=0)
            s += worst
        self.s = s
        self.floor = np.maximum(np.abs(self.o64), 1e-6 * max(float(np.abs(self.o64).max()), 1e-30))
        self.bound = 1e-5 * self.floor + np.abs(self.o32 - self.o64) + s
        # structurally below the horizon: both oracles 0 at d and the fp64 one at every perturbation
        self.dark = pert_zero & ~self.o32.any(axis=0) & ~self.o64.any(axis=0)
        self.loose = (self.bound > LOOSE * self.floor).any(axis=0)

    def ratio(self, img):
        """|img - o64| / bound per channel and pixel; img (C, h, w) or (C, h w)."""
        return np.abs(np.asarray(img, np.float64).reshape(self.o64.shape) - self.o64) / self.bound

    def check(self, img, loose_cap, what):
        """The bound on every pixel, exact zeros on the structurally dark ones, the loose cap;
        -> (worst ratio, loose pixels)."""
        img = np.asarray(img).reshape(self.o64.shape)
        assert not np.isnan(img).any(), f"{what}: NaN"
        r = self.ratio(img)
        nloose = int(self.loose.sum())
        print(f"{what}: worst ratio {r.max():.3f}, loose {nloose} of {self.loose.size}")
        assert nloose <= loose_cap * self.loose.size, f"{what}: {nloose} of {self.loose.size} pixels loose"
        bad = r > 1.0
        assert not bad.any(), (f"{what}: {int(bad.any(axis=0).sum())} of {self.loose.size} pixels over the bound, worst "
                               f"{r.max():.3g}x at pixel {int(np.argmax(r.max(axis=0)))}")
        lit = img[:, self.dark] != 0
        assert not lit.any(), f"{what}: {int(lit.any(axis=0).sum())} pixels below the horizon are not 0"
        return float(r.max()), nloose


def bake_images(frame):
    """Every image of the bake tests -> [(name, w, h, theta, phi, loose cap)]."""
    full = ((0.0, math.pi), (0.0, 2 * math.pi))
    out = [(f"sphere_{w}x{h}", w, h, *full, 0.0) for w, h in SPHERE_SIZES]
    out.append(("window", *WINDOW["size"], WINDOW["theta"], WINDOW["phi"], 0.0))
    out.append(("window_reversed", *WINDOW_REVERSED["size"], WINDOW_REVERSED["theta"], WINDOW_REVERSED["phi"], 0.0))
    st, sp = sun_window(frame)
    out += [(f"sun_{w}x{h}", w, h, st, sp, 0.03) for w, h in SUN_WINDOW_SIZES]
    return out


def bake_lists(variant):
    """The wavelength lists of a variant's bakes: {name: list or None}."""
    return {"rgb": None} if variant == "rgb" else {"nodes": NODES, "off_nodes": BAKE_OFF_NODES}
