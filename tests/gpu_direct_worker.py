"""Worker of tests/test_gpu_direct_shapes.py, and the calls both sides of its tests make: the six
direct-lighting kernels (sunsky_direct_{diffuse,conductor}_{rgb,spec}, sunsky_direct_diffuse_rays,
sunsky_direct_conductor_rays) through the Python wrappers (packed planes) and through the C ABI
(row strides above n, plane bases aligned to 4 bytes only, canaried outputs).

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every grid
is capped at one workgroup per CU):  gpu_direct_worker.py <n> <output directory>
runs every (variant, precision, frame) of COMBOS and saves each one's outputs (run_grid) to
<variant>_<precision>_<frame>.npz.  Exit 0 = all saved."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "mitsuba3-sunsky_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sunsky_amd as ss  # noqa: E402
from gpu_grid_stride_worker import EMITTER, NODES, OFF_NODES  # noqa: E402
from helpers import sphere_wo  # noqa: E402

FRAMES = ("identity", "rotated")
COMBOS = [(v, p, f) for v in ("rgb", "spectral") for p in ("fast", "reference") for f in FRAMES]
GOLD = dict(eta=(0.143, 0.374, 1.442), k=(3.983, 2.385, 1.603))    # as test_direct_conductor.GOLD
# (distribution, alpha): both distributions, each with an isotropic and an anisotropic alpha
CONDUCTORS = [("beckmann", 0.25), ("ggx", (0.08, 0.35)), ("ggx", 0.25), ("beckmann", (0.08, 0.35))]
CANARY = 0x5A5AA5A5      # the bit pattern (a finite float, 1.5e16) every output element holds before a strided call
PAD = 5                  # the strided calls' row stride is n + PAD
SCENES = ("base", "sky_only", "sun_only", "below_horizon")


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], dtype=np.float32)


def scene(frame="identity", name="base"):
    """EMITTER, or one of its degenerate forms: sky only (the sun-pick weight 1 - w_sky is 0),
    sun only (w_sky is 0), the sun 95 degrees from the zenith (below the horizon: black)."""
    d = dict(EMITTER)
    if name == "sky_only":
        d["sun_scale"] = 0.0
    elif name == "sun_only":
        d["sky_scale"] = 0.0
    elif name == "below_horizon":
        t, p = np.deg2rad(95.0), 0.7
        d["sun_direction"] = [float(np.cos(p) * np.sin(t)), float(np.sin(p) * np.sin(t)), float(np.cos(t))]
    elif name != "base":
        raise ValueError(name)
    if frame == "rotated":
        d["to_world"] = rot_x(0.35)
    return d


def emitter(variant, precision, frame="identity", name="base"):
    return ss.SunskyEmitter(scene(frame, name), variant, precision=precision)


def cap_step():
    """Points one grid-stride step covers at one workgroup per CU (one point per lane)."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 256


def batch_size():
    """Two and a half grid-stride steps at one workgroup per CU, plus 3: some lanes take three
    steps, some two (163 843 points on 256 CUs)."""
    step = cap_step()
    return 2 * step + step // 2 + 3


def bake_sizes():
    """(width, height) of the RGB (4 pixels per lane) and the spectral (1 pixel per lane) bake:
    more than two and a half steps of either kernel at one workgroup per CU."""
    items = 2 * cap_step() + cap_step() // 2
    return (1024, items // 256 + 1), (512, items // 512 + 1)


def normals(n, seed, axes=False):
    """test_direct_diffuse._gpu_normals (mostly facing the sky, some grazing); axes: the first six
    exactly +-z, +-x, +-y (the sign branch of coordinate_system, a frame with zero components)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v[:, 2] = np.abs(v[:, 2]) + 0.2
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    if axes:
        v[:6] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]]
    return v


def views(nrm, seed, below=0.03):
    """test_direct_conductor._gpu_views: per point a view direction in the normal's upper
    hemisphere (some grazing), a share `below` of them under the surface (black)."""
    rng = np.random.default_rng(seed)
    n = nrm.shape[0]
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    d = (v * nrm).sum(1)
    v = np.where((d < 0)[:, None], v - 2 * d[:, None] * nrm, v)
    flip = rng.random(n) < below
    v[flip] = v[flip] - 2 * (v[flip] * nrm[flip]).sum(1)[:, None] * nrm[flip]
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def inputs(n, spp, seed=41, axes=False):
    """numpy from a fixed seed (the same in the parent and in the child): normals and views
    (3, n), 4 wavelength planes, a reflectance plane, tracer verdicts (spp, n) uint8 in 0..3,
    and the directions / samples of sample_wavelengths."""
    rng = np.random.default_rng(seed)
    nrm = normals(n, seed + 1, axes)
    return dict(nrm=np.ascontiguousarray(nrm.T), wi=np.ascontiguousarray(views(nrm, seed + 2).T),
                lam=rng.uniform(360.0, 720.0, (4, n)).astype(np.float32),
                rho=rng.uniform(0.2, 0.9, n).astype(np.float32),
                vis=rng.integers(0, 4, (spp, n), dtype=np.uint8),
                wo=np.ascontiguousarray(sphere_wo(n, seed=seed + 3).T), ws=rng.random(n, dtype=np.float32))


def to_gpu(inp, m=None):
    """The inputs on the GPU; m: their first m points (every plane repacked)."""
    return {k: torch.from_numpy(np.ascontiguousarray(v[..., :m])).cuda() for k, v in inp.items()}


def run_direct(em, t, seed, spp, nlam=4, conductors=CONDUCTORS, vis=True, diffuse=True):
    """The six kernels' packed calls (the Python wrappers) -> {name: tensor}: direct_diffuse with
    a reflectance plane, direct_diffuse_rays, and per conductor direct_conductor and
    direct_conductor_rays without and with the BSDF weights.  vis: True = t["vis"], None =
    unoccluded, or a (spp, n) tensor.  Spectral emitters take the first nlam wavelength planes."""
    lam = t["lam"][:nlam].contiguous() if em.is_spectral else None
    v = t["vis"][:spp].contiguous() if vis is True else vis
    out = {}
    if diffuse:
        out["diffuse"] = em.direct_diffuse(t["nrm"], seed, spp, lam, t["rho"], visibility=v)
        out["diffuse_rays_em"], out["diffuse_rays_bs"] = em.direct_diffuse_rays(t["nrm"], seed, spp)
    for dist, alpha in conductors:
        key = f"conductor_{dist}_{'aniso' if np.ndim(alpha) else 'iso'}"
        out[key] = em.direct_conductor(t["nrm"], t["wi"], alpha, dist, GOLD["eta"], GOLD["k"], seed, spp, lam,
                                       visibility=v)
        e0, b0 = em.direct_conductor_rays(t["nrm"], t["wi"], alpha, dist, seed, spp)
        e1, b1, w1 = em.direct_conductor_rays(t["nrm"], t["wi"], alpha, dist, seed, spp, GOLD["eta"], GOLD["k"])
        out.update({key + "_rays_em": e0, key + "_rays_bs": b0, key + "_raysw_em": e1, key + "_raysw_bs": b1,
                    key + "_raysw_bw": w1})
    return out


GRID_SPP, GRID_SEED = 2, 77
GRID_CONDUCTORS = CONDUCTORS[:2]


def run_grid(variant, precision, frame, inp):
    """What the capped-grid test compares -> {name: numpy array}: the six direct kernels with
    visibility (spectral: at 4 and at 3 wavelengths), sample_wavelengths, and bake_latlong
    (spectral: at the 11 nodes and at 5 off-node wavelengths) at bake_sizes()."""
    em = emitter(variant, precision, frame)
    t = to_gpu(inp)
    out = run_direct(em, t, GRID_SEED, GRID_SPP, 4, GRID_CONDUCTORS)
    if em.is_spectral:
        out.update({k + "_nlam3": v for k, v in run_direct(em, t, GRID_SEED, GRID_SPP, 3, GRID_CONDUCTORS).items()
                    if "rays" not in k})
    out["wavelengths_lam"], out["wavelengths_w"] = em.sample_wavelengths(
        ss.SurfaceInteraction3f(wi=-t["wo"]), t["ws"] if em.is_spectral else None)
    (wr, hr), (wsp, hs) = bake_sizes()
    if em.is_spectral:
        out["bake_nodes"] = em.bake_latlong(wsp, hs, wavelengths=NODES)
        out["bake_off_nodes"] = em.bake_latlong(wsp, hs, wavelengths=OFF_NODES)
    else:
        out["bake"] = em.bake_latlong(wr, hr)
    torch.cuda.synchronize()
    return {k: v.contiguous().cpu().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- the C ABI with strides
class Planes:
    """rows x n elements at a row stride of n + PAD, the base one element (fp32: 4 bytes, so
    4-byte aligned only; uint8: 1 byte) into an allocation with 8 guard elements at either end.
    src (rows, n) fills the rows; without it every element holds CANARY (an output)."""

    def __init__(self, rows, n, src=None, dtype=torch.float32):
        self.rows, self.n, self.stride = rows, n, n + PAD
        size = 8 + 1 + rows * self.stride + 8
        if dtype == torch.float32:
            self.raw = torch.full((size,), CANARY, dtype=torch.int32, device="cuda")
            self.buf = self.raw.view(torch.float32)
        else:
            self.raw = self.buf = torch.full((size,), 0xA5, dtype=dtype, device="cuda")
        self.body = self.buf[9:9 + rows * self.stride].view(rows, self.stride)
        assert self.body.data_ptr() % 16 != 0 and self.raw.data_ptr() % 16 == 0
        if src is not None:
            self.body[:, :n] = src
        self.written = torch.zeros(size, dtype=torch.bool, device="cuda")

    def ptr(self, row=0):
        return self.body[row].data_ptr()

    def v3(self, row=0, cls=None):
        return (cls or ss._capi.Vec3In)(self.ptr(row), self.ptr(row + 1), self.ptr(row + 2))

    def columns(self, rows=None):
        """Columns [0, n) of the first `rows` rows: what a call may write."""
        rows = self.rows if rows is None else rows
        self.written[9:9 + self.rows * self.stride].view(self.rows, self.stride)[:rows, :self.n] = True
        return self.body[:rows, :self.n]

    def untouched(self):
        """Elements outside every columns() taken so far that no longer hold the canary."""
        assert self.raw.dtype == torch.int32, "only fp32 planes are canaried (uint8 planes are inputs)"
        return int(((self.raw != CANARY) & ~self.written).sum())


def _fa(v):
    return (ctypes.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(v, np.float32), (3,))])


def run_direct_strided(em, inp, seed, spp, nlam=4, conductors=CONDUCTORS):
    """run_direct's calls through ss.lib() with every stride n + PAD (out_stride, wl_stride,
    vis_stride, ray_stride), every input plane base off 16-byte alignment and canaried outputs
    -> ({name: tensor of columns [0, n)}, {name: number of padding / guard / unused-row elements
    that lost the canary}).  Spectral outputs are allocated with four rows whatever nlam."""
    lib, h, st = ss.lib(), em._h, em._stream()
    spec = em.is_spectral
    n = inp["nrm"].shape[1]
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    nrm, wi = Planes(3, n, g(inp["nrm"])), Planes(3, n, g(inp["wi"]))
    lam = Planes(4, n, g(inp["lam"])) if spec else None
    rho = Planes(1, n, g(inp["rho"])[None])
    vis = Planes(spp, n, g(inp["vis"][:spp]), dtype=torch.uint8)
    stride = n + PAD
    lam_args = (lam.ptr(), nlam, stride) if spec else (None, 0, 0)
    nc = nlam if spec else 3
    planes, used = {}, {}

    def alloc(name, rows, rows_used=None):
        planes[name], used[name] = Planes(rows, n), rows if rows_used is None else rows_used
        return planes[name]

    # a ray plane set (3, spp, n): component c at rows [c spp, (c + 1) spp), sample s at row s of them
    ray3 = lambda p: ss._capi.Vec3Out(p.ptr(0), p.ptr(spp), p.ptr(2 * spp))   # noqa: E731
    o = alloc("diffuse", 4 if spec else 3, nc)
    ss._capi.check(lib.sunsky_direct_diffuse(h, nrm.v3(), rho.ptr(), *lam_args, seed, spp, vis.ptr(), stride, n,
                                             o.ptr(), stride, st))
    e, b = alloc("diffuse_rays_em", 3 * spp), alloc("diffuse_rays_bs", 3 * spp)
    ss._capi.check(lib.sunsky_direct_diffuse_rays(h, nrm.v3(), seed, spp, n, ray3(e), ray3(b), stride, st))
    for dist, alpha in conductors:
        key = f"conductor_{dist}_{'aniso' if np.ndim(alpha) else 'iso'}"
        au, av = (alpha, alpha) if np.ndim(alpha) == 0 else alpha
        d = {"beckmann": 0, "ggx": 1}[dist]
        eta, k = _fa(GOLD["eta"]), _fa(GOLD["k"])
        o = alloc(key, 4 if spec else 3, nc)
        ss._capi.check(lib.sunsky_direct_conductor_aniso(h, nrm.v3(), wi.v3(), d, au, av, eta, k, *lam_args, seed, spp,
                                                         vis.ptr(), stride, n, o.ptr(), stride, st))
        e, b = alloc(key + "_rays_em", 3 * spp), alloc(key + "_rays_bs", 3 * spp)
        ss._capi.check(lib.sunsky_direct_conductor_rays_aniso(h, nrm.v3(), wi.v3(), d, au, av, None, None, seed, spp, n,
                                                              ray3(e), ray3(b), None, stride, st))
        e, b = alloc(key + "_raysw_em", 3 * spp), alloc(key + "_raysw_bs", 3 * spp)
        w = alloc(key + "_raysw_bw", (1 if spec else 3) * spp)
        ss._capi.check(lib.sunsky_direct_conductor_rays_aniso(h, nrm.v3(), wi.v3(), d, au, av, eta, k, seed, spp, n,
                                                              ray3(e), ray3(b), w.ptr(), stride, st))
    torch.cuda.synchronize()
    out, lost = {}, {}
    for name, p in planes.items():
        c = p.columns(used[name]).clone()
        out[name] = c.reshape(-1, spp, n) if "rays" in name else c   # rays: (3 | C, spp, n), as the wrappers return
        lost[name] = p.untouched()
    return out, lost


def main():
    n, outdir = int(sys.argv[1]), sys.argv[2]
    torch.cuda.set_device(0)
    inp = inputs(n, GRID_SPP)
    for variant, precision, frame in COMBOS:
        np.savez(os.path.join(outdir, f"{variant}_{precision}_{frame}.npz"), **run_grid(variant, precision, frame, inp))
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
