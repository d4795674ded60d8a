"""Plain numpy fp64 restatements and the input generators of the sampling-shape tests
(tests/test_sampling_shapes_cpu.py, tests/test_gpu_sampling_shapes.py and its worker
tests/gpu_sampling_worker.py, tools/sampling_shapes_measure.py).  No GPU and no oracle in here.

ray_origin(): the origin of sample_ray (sunsky.cpp:354-397) from a given fp32 ray direction d
(world frame) and its sample2, all in fp64:

    sg = copysign(1, d.z);  a = -1 / (sg + d.z);  b = d.x d.y a          coordinate_system(d)
    s  = (d.x^2 a sg + 1,  b sg,  -d.x sg);   t = (b,  d.y^2 a + sg,  -d.y)
    (x, y) = 2 sample2 - 1                                               warp.h:54-90
    r = the one of x, y with the larger magnitude (y if |x| < |y|), rp the other
    phi = pi/4 rp / r   (pi/2 - that if |x| < |y|; 0 at x = y = 0);  off = (r cos phi, r sin phi)
    o = c + R (s off.x + t off.y - d)

origin_unit(): the unit 2^-24 (|c_i| + 2 R) per component the origin bound is stated in: an fp32
origin is a sum of terms of magnitude |c_i| and at most 2 R, each rounded once or twice."""
import numpy as np

from helpers import angles_dict, sphere_wo, sun_cone_wo

PERMUTE = np.array([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
BBOX = ([-1, -2, -3], [3, 2, 1])                    # set_scene of the existing bitwise tests
# (centre, radius) of the two sample_ray scenes; every value is exact in fp32
SCENES = {"small": ((1.0, 0.0, -1.0), float(np.float32(3.7))), "large": ((1e4, -2e3, 5e2), 1e3)}
NODES = np.arange(320, 721, 40, dtype=np.float32)   # the 11 model wavelengths
EDGE_LAMBDA = np.array([360, 720, 300, 800, np.nextafter(np.float32(720), np.float32(0)), 359.9], np.float32)
MAX_LAMBDA = 16                                     # kMaxLambdaPerRay
SKY_ROWS, SUN_ROWS = slice(768, 1536), slice(1536, 2304)   # whole windows of 4 x 64 and of 3 x 64 samples
MASKS = ("none", "all_true", "all_false", "mixed")
SIZES = (1, 65, 191, 193, 255, 257, 4099)
PREFIX_N, PREFIX_M = 4099, (1, 2, 63, 64, 65, 191, 192, 193, 255, 256, 257, 4099)


def emitter_dict(frame="rotated"):
    """The emitter of the existing bitwise tests (test_wave_sorted_rgb_kernels_bitwise_vs_unsorted):
    T = 3, the sun 30 degrees above the horizon; rotated: to_world an axis permutation."""
    d = angles_dict(3.0, 1.1, np.deg2rad(60), 0.3, 1.0, 1.0)
    if frame == "rotated":
        d["to_world"] = PERMUTE.copy()
    elif frame != "identity":
        raise ValueError(frame)
    return d


def sweep_dict(case):
    """An emitter of test_gpu_parity.SAMPLING_SWEEP: (turbidity, albedo, elevation deg, azimuth
    deg, sky_scale, sun_scale)."""
    turb, albedo, elev, az, sky_scale, sun_scale = case
    return angles_dict(turb, np.deg2rad(az), np.deg2rad(90.0 - elev), albedo, sky_scale, sun_scale)


def special_samples(w_sky):
    """u.x at w_sky and its two fp32 neighbours, 0 and 1 - 2^-24; all inside [0, 1)."""
    w = np.float32(w_sky)
    s = np.array([w, np.nextafter(w, np.float32(0)), np.nextafter(w, np.float32(1)), 0.0,
                  np.nextafter(np.float32(1), np.float32(0))], np.float32)
    return np.clip(s, 0, np.nextafter(np.float32(1), np.float32(0)))


# sample2 at the disk's centre, the square's corners and its edge midpoints (|x| = |y| and x or
# y = 0: the branch switch and the zero of square_to_uniform_disk_concentric)
_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
DISK_SPECIALS = np.array([[0.5, 0.5], [0, 0], [0, _ONE], [_ONE, 0], [_ONE, _ONE], [0.5, 0], [0.5, _ONE], [0, 0.5],
                          [_ONE, 0.5], [0.25, 0.25], [0.25, 0.75], [0.75, 0.25]], np.float32)


def mask(kind, n, seed=3):
    """none -> None.  mixed: about 70 % set, and both values inside every row of 64 samples (a
    wave's row of a window) that has two samples or more."""
    if kind == "none":
        return None
    if kind == "all_true":
        return np.ones(n, bool)
    if kind == "all_false":
        return np.zeros(n, bool)
    if kind != "mixed":
        raise ValueError(kind)
    m = np.random.default_rng(seed).random(n) < 0.7
    for k, base in enumerate(range(0, n, 64)):
        rows = min(64, n - base)
        if rows >= 2:
            a = k % rows
            m[base + a], m[base + (a + 1) % rows] = False, True
    return m


def inputs(n, w_sky, seed=71, sun_dir=None):
    """numpy from a fixed seed (the same in a parent and in its child process): u (2, n) the
    direction sample with the specials first and, from 2304 samples on, an all-sky and an all-sun
    stretch that cover whole windows of both kinds; s2 (2, n) the origin sample with DISK_SPECIALS
    first; ws (n,) the wavelength sample; lam (16, n) in [360, 720] with the 11 nodes, 360, 720
    and wavelengths outside the range among them; p (3, n) interaction positions; wo (3, n) unit
    directions, every eighth inside the sun disc when sun_dir (world) is given."""
    rng = np.random.default_rng(seed)
    u = rng.random((2, n), dtype=np.float32)
    sp = special_samples(w_sky)
    k = min(n, sp.size)
    u[0, :k] = sp[:k]
    w = np.float32(w_sky)
    if n >= SUN_ROWS.stop:
        u[0, SKY_ROWS] = np.minimum(u[0, SKY_ROWS] * w, np.nextafter(w, np.float32(0))) if w > 0 else u[0, SKY_ROWS]
        u[0, SUN_ROWS] = np.minimum(w + (1 - w) * u[0, SUN_ROWS], np.float32(_ONE))
    s2 = rng.random((2, n), dtype=np.float32)
    k = min(n, len(DISK_SPECIALS))
    s2[:, :k] = DISK_SPECIALS[:k].T
    lam = rng.uniform(360.0, 720.0, (MAX_LAMBDA, n)).astype(np.float32)
    if n >= 1300:
        lam[:, 1100:1111] = NODES[None, :]
        lam[:, 1200:1206] = EDGE_LAMBDA[None, :]
        lam[:4, 1210:1216] = np.stack([np.roll(EDGE_LAMBDA, j) for j in range(4)])   # rows that differ
    wo = sphere_wo(n, seed=seed + 1)
    if sun_dir is not None:
        wo[::8] = sun_cone_wo(len(wo[::8]), sun_dir, np.deg2rad(0.2), seed=seed + 2)
    return dict(u=u, s2=s2, ws=rng.random(n, dtype=np.float32), lam=lam,
                p=(rng.standard_normal((3, n)) * 10).astype(np.float32), wo=np.ascontiguousarray(wo.T))


def ray_inputs(n, w_sky, seed=83):
    """sample_ray's samples for the reference tests -> (ws (n,), s2 (n, 2), s3 (n, 2))."""
    inp = inputs(n, w_sky, seed)
    return inp["ws"], np.ascontiguousarray(inp["s2"].T), np.ascontiguousarray(inp["u"].T)


# ---------------------------------------------------------------- the origin of a ray
def disk(s2):
    """square_to_uniform_disk_concentric (warp.h:54-90), fp64 -> (off (n, 2), r (n,))."""
    s2 = np.asarray(s2, np.float64)
    x, y = 2.0 * s2[:, 0] - 1.0, 2.0 * s2[:, 1] - 1.0
    q = np.abs(x) < np.abs(y)
    r, rp = np.where(q, y, x), np.where(q, x, y)
    zero = (x == 0) & (y == 0)
    phi = 0.25 * np.pi * rp / np.where(zero, 1.0, r)
    phi = np.where(q, 0.5 * np.pi - phi, phi)
    phi = np.where(zero, 0.0, phi)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], 1), r


def frame(d):
    """coordinate_system(d) (vector.h), fp64 -> (s, t), each (n, 3)."""
    d = np.asarray(d, np.float64)
    sg = np.copysign(1.0, d[:, 2])
    a = -1.0 / (sg + d[:, 2])
    b = d[:, 0] * d[:, 1] * a
    s = np.stack([d[:, 0] * d[:, 0] * a * sg + 1.0, b * sg, -d[:, 0] * sg], 1)
    t = np.stack([b, d[:, 1] * d[:, 1] * a + sg, -d[:, 1]], 1)
    return s, t


def ray_origin(d, s2, center, radius):
    """(n, 3) fp64 origins of the rays with directions d (n, 3) and origin samples s2 (n, 2)."""
    d = np.asarray(d, np.float64)
    off, _ = disk(s2)
    s, t = frame(d)
    return np.asarray(center, np.float64)[None, :] + float(radius) * (s * off[:, :1] + t * off[:, 1:] - d)


def origin_unit(center, radius):
    """(3,) 2^-24 (|c_i| + 2 R)."""
    return 2.0 ** -24 * (np.abs(np.asarray(center, np.float64)) + 2.0 * float(radius))


def origin_ratio(o, d, s2, center, radius):
    """max over rays and components of |o - ray_origin(d)| in origin_unit()s."""
    err = np.abs(np.asarray(o, np.float64) - ray_origin(d, s2, center, radius))
    return float((err / origin_unit(center, radius)[None, :]).max())


def origin_invariants(o, d, s2, center, radius):
    """With q = (o - c) / R + d (the ray's offset on its disk): (max |q . d|, max ||q| - |r||),
    which do not depend on the frame (s, t) chosen around d."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    q = (o - np.asarray(center, np.float64)[None, :]) / float(radius) + d
    _, r = disk(s2)
    return float(np.abs((q * d).sum(1)).max()), float(np.abs(np.linalg.norm(q, axis=1) - np.abs(r)).max())


def ulps(a, b):
    """Largest distance of two finite fp32 arrays in units in the last place."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max()) if np.size(a) else 0
