"""Finite-difference reference for d eval / d wi (tests/test_gpu_eval_dir_ad.py): 4-point central
differences of the fp64 oracle, numpy only.

The oracle takes fp32 directions, so the stencils step ON the sphere: the points of a lane
wo along a unit tangent t (t . wo = 0) are wo cos(s) + t sin(s), rounded to fp32; the
derivative along the arc at s = 0 is grad f . t.  (Axis steps from an off-sphere base are
wrong: unit_angle switches branch at dot = 0 and its two branches differ by ~ |wo| - 1 off the
sphere, and the disc test dot >= cos_cutoff is sensitive to scale.)  Radial steps wo (1 + s)
are used on sky lanes with gamma > 0.1 only: closer lanes scale into the disc mask.

The bar is tests/test_eval_jvp.py check()'s constants applied to each lane's gradient magnitude
per channel, G = sqrt(sum_t fd_t^2) over the lane's tested tangents:
    |x_t - fd_t| <= 2e-3 G_i + 1e-4 max_i G_i.
The fp32 rounding of a stencil point perturbs f by ~ |grad f| 3e-8 whatever the direction t,
so a bar relative to a small directional derivative alone would measure the oracle's input
rounding, not the kernel."""
import contextlib
import functools
import math

import numpy as np

import oracle as O
from helpers import angles_dict, hemisphere_wo

H_SKY, H_DISC = 2e-3, 4e-4
SELF_SKY, SELF_DISC = 0.1, 0.5      # stencil at h vs h / 2, as a fraction of the bar
N_SKY_DRAW, N_DISC = 4096, 2048

SCENES = {
    "mid": angles_dict(3.4, 0.6, math.pi / 2 - math.radians(40), 0.3, 1.0, 1.0),
    "low": angles_dict(6.5, 0.6, math.pi / 2 - math.radians(12), 0.3, 1.0, 1.0),
}


@contextlib.contextmanager
def few_threads(n=16):
    """The oracle with at most n OpenMP threads: these batches are a few thousand lanes, and an
    earlier test of a whole-suite run may have set one thread per CPU of the machine
    (O.set_threads), which on a share of the machine's CPUs costs seconds per call here."""
    before = O.get_threads()
    O.set_threads(max(1, min(before, n)))
    try:
        yield
    finally:
        O.set_threads(before)


def xform(key, scene="mid"):
    """3 x 3 linear part of to_world: identity, a rotation, a rotation times a non-uniform scale.
    The scale D keeps the scene's sun direction s at unit length, |D s| = 1: the emitter
    normalises sun_direction in the world and takes it to its frame with to_world^-1 as is, so
    any other scale leaves it (like the reference) with a non-unit sun vector in unit_angle,
    whose branch switch at dot = 0 then jumps -- not a function to differentiate."""
    if key == "ident":
        return np.eye(3)
    a, b = 0.7, -0.4
    rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    rz = np.array([[math.cos(b), -math.sin(b), 0], [math.sin(b), math.cos(b), 0], [0, 0, 1]])
    m = rz @ rx
    if key == "scaled":
        sx, sy, sz = SCENES[scene]["sun_direction"]
        m = m @ np.diag([1.25, 0.8, math.sqrt(1.0 - (1.25 * sx) ** 2 - (0.8 * sy) ** 2) / sz])
    return m.astype(np.float32).astype(np.float64)   # the bits the emitter and the oracle are given


def scene_dict(scene, xf):
    d = dict(SCENES[scene])
    if xf != "ident":
        # the SCENES directions are in the emitter's frame: sun_direction is a world vector
        m = xform(xf, scene)
        d["sun_direction"] = [float(v) for v in m @ np.array(d["sun_direction"])]
        t = np.eye(4, dtype=np.float32)
        t[:3, :3] = m
        d["to_world"] = t
    return d


def tangent_frame(wo):
    """Two unit tangents per lane, orthogonal to wo (n, 3) and to each other."""
    a = np.where(np.abs(wo[:, 2:3]) < 0.9, [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]])
    t1 = np.cross(wo, a)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    return t1, np.cross(wo, t1)


def sky_lanes(sun_local, seed):
    """Upper-hemisphere unit directions (fp64) with cos theta > 0.02 and gamma > 0.1."""
    wo = hemisphere_wo(N_SKY_DRAW, seed=seed).astype(np.float64)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    gamma = np.arccos(np.clip(wo @ sun_local, -1, 1))
    keep = (wo[:, 2] > 0.02) & (gamma > 0.1)
    assert keep.mean() >= 0.95, keep.mean()   # no more than 5 % dropped
    return wo[keep]


def disc_lanes(sun_local, half_aperture, seed):
    """Directions with gamma uniform in [0.25, 0.5] of the half aperture (the lower bound is
    the existing disc test's, for the fp32 chord cancellation; the upper keeps the 2 h stencil
    inside the disc), any azimuth about the sun."""
    rng = np.random.default_rng(seed)
    s = sun_local / np.linalg.norm(sun_local)
    e1, e2 = tangent_frame(s[None])
    g = half_aperture * rng.uniform(0.25, 0.5, N_DISC)
    ph = rng.uniform(0, 2 * np.pi, N_DISC)
    assert g.max() + 2 * H_DISC < half_aperture
    return (np.cos(g)[:, None] * s + np.sin(g)[:, None] * (np.cos(ph)[:, None] * e1 + np.sin(ph)[:, None] * e2))


def _eval(o, m, pts, lam):
    """Oracle eval at local directions pts (n, 3) -> (k, n) fp64."""
    wi = (-(pts @ m.T)).astype(np.float32)
    v = o.eval(wi, lam)
    return v if o.spectral else v.T


def d4(f, h):
    """4-point central difference of f(s) at 0 with step h."""
    return (8.0 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12.0 * h)


def stencils(o, m, wo, tangents, lam, h, radial):
    """-> fd at h and at h / 2, each (T, k, n): along every tangent of `tangents` on the sphere
    and, if radial, along wo itself."""
    paths = [(lambda s, t=t: wo * np.cos(s) + t * np.sin(s)) for t in tangents]
    if radial:
        paths.append(lambda s: wo * (1.0 + s))
    out = []
    for step in (h, h / 2):
        cache = {}

        def f(s, p):
            if (s, id(p)) not in cache:
                cache[(s, id(p))] = _eval(o, m, p(s), lam)
            return cache[(s, id(p))]
        out.append(np.stack([d4(lambda s, p=p: f(s, p), step) for p in paths]))
    return out


def bar(fd):
    """(T, k, n) -> the bound (k, n): 2e-3 G + 1e-4 max over the lanes of G, per channel."""
    g = np.sqrt((fd ** 2).sum(axis=0))
    return 2e-3 * g + 1e-4 * g.max(axis=-1, keepdims=True)


def worst(x, fd):
    """Worst |x - fd| over the bar."""
    return float((np.abs(x - fd) / bar(fd)[None]).max())


@functools.lru_cache(maxsize=None)
def reference(scene, variant, xf, disc=True):
    """The lanes, tangents and stencils of one configuration, computed once:
    {"sky": {...}, "disc": {...}} with wo (n, 3) fp64 unit local directions, dirs (T, n, 3) the
    local tangents (the radial one last on sky lanes), lam (4, n) or None, fd / fd2 (T, k, n)
    the stencils at h and h / 2, and d, m the scene dict and to_world's linear part."""
    with few_threads():
        return _reference(scene, variant, xf, disc)


def _reference(scene, variant, xf, disc):
    d = scene_dict(scene, xf)
    m = xform(xf, scene)
    o32 = O.Oracle(d, variant, "jit", "f32")
    o64 = O.Oracle(d, variant, "jit", "f64")
    inf = o32.info()
    sun = np.asarray(inf["sun_dir_local"], np.float64)
    out = {"d": d, "m": m, "sun_local": sun, "cos_cutoff": float(inf["cos_cutoff"])}
    groups = [("sky", sky_lanes(sun, 71), H_SKY, True)]
    if disc:
        groups.append(("disc", disc_lanes(sun, math.acos(inf["cos_cutoff"]), 72), H_DISC, False))
    for gi, (name, wo, h, radial) in enumerate(groups):
        n = wo.shape[0]
        lam = None
        if variant == "spectral":
            lam = np.random.default_rng(73 + gi).uniform(330, 710, (4, n)).astype(np.float32)
        t1, t2 = tangent_frame(wo)
        fd, fd2 = stencils(o64, m, wo, [t1, t2], lam, h, radial)
        dirs = np.stack([t1, t2] + ([wo] if radial else []))
        out[name] = dict(wo=wo, dirs=dirs, lam=lam, fd=fd, fd2=fd2)
    return out


def assert_self_consistent(ref, group, what=""):
    """The oracle's own stencils at h and h / 2 agree to a fraction of the bar."""
    g = ref[group]
    r = worst(g["fd2"], g["fd"])
    limit = SELF_SKY if group == "sky" else SELF_DISC
    print(f"{what} {group}: oracle stencil h vs h/2, worst {r:.3f} of the bar (limit {limit})")
    assert r <= limit, (what, group, r)
    return r
