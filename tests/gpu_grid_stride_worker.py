"""Worker of tests/test_gpu_grid_stride.py, and the calls both sides of that test make.

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every
grid is capped at one workgroup per CU):  gpu_grid_stride_worker.py <n> <output directory>
runs every (variant, precision) and saves each one's outputs to <variant>_<precision>.npz.
Exit 0 = all saved."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "mitsuba3-sunsky_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sunsky_amd as ss  # noqa: E402
from helpers import angles_dict, sphere_wo, sun_cone_wo  # noqa: E402

COMBOS = [(v, p) for v in ("rgb", "spectral") for p in ("fast", "reference")]
EMITTER = angles_dict(3.0, 0.7, np.deg2rad(55.0), 0.3, 1.0, 1.0)
NODES = [float(x) for x in range(320, 721, 40)]     # the 11 model wavelengths: the node kernel
OFF_NODES = [350.0, 412.5, 555.0, 633.25, 700.0]    # the general broadcast kernel


def batch_size():
    """Two and a half grid-stride steps of a 4-directions-per-lane kernel at one workgroup per
    CU, plus a 3-element scalar tail: some lanes take three steps, some two."""
    step = torch.cuda.get_device_properties(0).multi_processor_count * 256 * 4
    return 2 * step + step // 2 + 3


def inputs(n, seed=33):
    """numpy from a fixed seed: the same in the parent and in the child."""
    rng = np.random.default_rng(seed)
    wo = sphere_wo(n, seed=seed)
    # every eighth direction inside the sun disc (within 0.2 deg; half aperture 0.268 deg)
    wo[::8] = sun_cone_wo(len(wo[::8]), EMITTER["sun_direction"], np.deg2rad(0.2), seed=seed + 1)
    return dict(wo=np.ascontiguousarray(wo.T),
                u=rng.random((2, n), dtype=np.float32), u3=rng.random((2, n), dtype=np.float32),
                ws=rng.random(n, dtype=np.float32), p=rng.standard_normal((3, n)).astype(np.float32),
                lam=(360.0 + 360.0 * rng.random((4, n), dtype=np.float32)).astype(np.float32))


def _pitched(rows, n, src=None):
    """(rows, n) fp32 planes on the GPU at a pitch of n rounded up to 4 floats: every plane
    starts 16-byte aligned, as the 4-directions-per-lane kernels need (a packed (rows, n)
    tensor with n % 4 == 3 would send the whole batch to the scalar kernels)."""
    pitch = (n + 3) & ~3
    t = torch.zeros((rows, pitch), dtype=torch.float32, device="cuda")
    if src is not None:
        t[:, :n] = torch.from_numpy(src).cuda()
    assert t.data_ptr() % 16 == 0 and pitch % 4 == 0 and n % 4 == 3 and n > 4
    return t


def _v3(t):
    return ss._capi.Vec3In(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())


def run(variant, precision, inp):
    """Every batch entry point whose grid the kernel table sizes -> {name: numpy array}.
    eval, eval_direction, pdf_direction and eval_spectral_broadcast go through the C ABI with
    pitched planes, so that one call is a 4-per-lane body of n - 3 and a scalar tail of 3;
    eval_jvp (one lane per direction) along a turbidity and a sun_direction tangent."""
    spec = variant == "spectral"
    em = ss.SunskyEmitter(EMITTER, variant, precision=precision)
    lib, h, st = ss.lib(), em._h, em._stream()
    n = inp["wo"].shape[1]
    pitch = (n + 3) & ~3
    t = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    wo, wi = _pitched(3, n, inp["wo"]), _pitched(3, n, -inp["wo"])
    lam = t["lam"] if spec else None
    lam_p = _pitched(4, n, inp["lam"]) if spec else None
    out = {}

    def eval_call(fn, dirs):
        o = _pitched(4 if spec else 3, n)
        ss._capi.check(fn(h, _v3(dirs), lam_p.data_ptr() if spec else None, 4 if spec else 0, pitch if spec else 0,
                          None, n, o.data_ptr(), pitch, st))
        return o[:, :n]

    out["eval"] = eval_call(lib.sunsky_eval, wi)
    out["eval_direction"] = eval_call(lib.sunsky_eval_direction, wo)
    pdf = _pitched(1, n)
    ss._capi.check(lib.sunsky_pdf_direction(h, _v3(wo), None, n, pdf.data_ptr(), st))
    out["pdf_direction"] = pdf[0, :n]
    ds, w = em.sample_direction(ss.Interaction3f(wavelengths=lam), t["u"], positions=False)
    out.update(lean_d=ds.d, lean_pdf=ds.pdf, lean_w=w)
    ds, w = em.sample_direction(ss.Interaction3f(p=t["p"], wavelengths=lam), t["u"])
    out.update(pos_d=ds.d, pos_pdf=ds.pdf, pos_dist=ds.dist, pos_p=ds.p, pos_w=w)
    ray, rw = em.sample_ray(0.0, t["ws"] if spec else None, t["u"], t["u3"])
    out.update(ray_o=ray.o, ray_d=ray.d, ray_lam=ray.wavelengths, ray_w=rw)
    if spec:
        for name, wl in (("bcast_nodes", NODES), ("bcast_off_nodes", OFF_NODES)):
            o = _pitched(len(wl), n)
            ss._capi.check(lib.sunsky_eval_spectral_broadcast(h, _v3(wi), (ctypes.c_float * len(wl))(*wl), len(wl), None,
                                                              n, o.data_ptr(), pitch, st))
            out[name] = o[:, :n]
    # forward-mode AD: its grid is eval's (grid_for); the precision does not select a kernel
    si = ss.SurfaceInteraction3f(wi=-t["wo"], wavelengths=lam)
    for name, param, tangent in (("jvp_turbidity", "turbidity", [1.0]), ("jvp_sun", "sun_direction", [0.3, -0.2, 0.5])):
        out[name + "_val"], out[name + "_dval"] = em.eval_jvp(si, param, tangent)
    torch.cuda.synchronize()
    return {k: v.contiguous().cpu().numpy() for k, v in out.items()}


def main():
    n, outdir = int(sys.argv[1]), sys.argv[2]
    torch.cuda.set_device(0)
    inp = inputs(n)
    for variant, precision in COMBOS:
        np.savez(os.path.join(outdir, f"{variant}_{precision}.npz"), **run(variant, precision, inp))
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
