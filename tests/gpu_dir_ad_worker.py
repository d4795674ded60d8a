"""Worker of tests/test_gpu_eval_dir_ad.py::test_outputs_do_not_depend_on_the_grid, and the
calls both sides of that test make.

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every
grid is capped at one workgroup per CU):  gpu_dir_ad_worker.py <n> <output directory>
runs eval_jvp_dir and eval_vjp_dir for both variants and saves each variant's outputs to
<variant>.npz.  Exit 0 = all saved."""
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

VARIANTS = ("rgb", "spectral")
EMITTER = angles_dict(3.0, 0.7, np.deg2rad(55.0), 0.3, 1.0, 1.0)


def batch_size():
    """Two and a half grid-stride steps of a one-ray-per-lane kernel at one workgroup per CU,
    plus 3: some lanes take three steps, some two, and the last workgroup is ragged."""
    step = torch.cuda.get_device_properties(0).multi_processor_count * 256
    return 2 * step + step // 2 + 3


def inputs(n, seed=43):
    """numpy from a fixed seed: the same in the parent and in the child."""
    rng = np.random.default_rng(seed)
    wo = sphere_wo(n, seed=seed)
    # every eighth direction inside the sun disc (within 0.2 deg; half aperture 0.268 deg)
    wo[::8] = sun_cone_wo(len(wo[::8]), EMITTER["sun_direction"], np.deg2rad(0.2), seed=seed + 1)
    return dict(wi=np.ascontiguousarray(-wo.T), d_wi=rng.standard_normal((3, n)).astype(np.float32),
                cot=rng.standard_normal((4, n)).astype(np.float32),
                lam=(360.0 + 360.0 * rng.random((4, n), dtype=np.float32)).astype(np.float32))


def run(variant, inp):
    """The four kernels' outputs -> {name: numpy array}."""
    spec = variant == "spectral"
    em = ss.SunskyEmitter(EMITTER, variant)
    t = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    si = ss.SurfaceInteraction3f(wi=t["wi"], wavelengths=t["lam"] if spec else None)
    val, dval = em.eval_jvp_dir(si, t["d_wi"])
    grad = em.eval_vjp_dir(si, t["cot"] if spec else t["cot"][:3].contiguous())
    torch.cuda.synchronize()
    return {"val": val.cpu().numpy(), "dval": dval.cpu().numpy(), "grad": grad.cpu().numpy()}


def main():
    n, outdir = int(sys.argv[1]), sys.argv[2]
    torch.cuda.set_device(0)
    inp = inputs(n)
    for variant in VARIANTS:
        np.savez(os.path.join(outdir, f"{variant}.npz"), **run(variant, inp))
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
