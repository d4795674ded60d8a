"""Worker of tests/test_gpu_sequence_irradiance_grad.py's child-process tests, and the calls both
sides of them make.

As a program (a fresh child process, so that an environment variable the library reads once or
at prepare time takes effect):
    gpu_sequence_irradiance_grad_worker.py grid <n> <output directory>
        irradiance_vjp of both variants at a 64 x 256 table over n receivers; started with
        SUNSKY_AMD_BLOCKS_PER_CU=1, so that every grid-stride loop takes several steps
    gpu_sequence_irradiance_grad_worker.py cap <n> <output directory>
        the same call at a 16 x 32 table; started with a lowered workspace bound
saves <variant>_normals.npy and <variant>_weights.npy.  Exit 0 = all saved."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "mitsuba3-sunsky_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sunsky_amd as ss  # noqa: E402
from sequence_cases import LAMBDAS, TURBIDITY, WEIGHTS, base_dict, frame_dirs  # noqa: E402
from gpu_sequence_irradiance_worker import sphere_normals  # noqa: E402

VARIANTS = ("rgb", "spectral")
SIZES = {"grid": (64, 256), "cap": (16, 32)}
CAP_FLOATS = 3200   # 16 x 32, K = 5: two rows of RGB's 3 x 517 floats, one row of the spectral 5 x 517


def grid_batch_size():
    """Two receivers per lane of the normal kernel: two and a half grid-stride steps at one
    workgroup per CU, plus an odd remainder.  The adjoint kernel then has 64 slices x 17 tiles
    work items (x 2 passes, spectral) for its CU-count workgroups."""
    step = torch.cuda.get_device_properties(0).multi_processor_count * 256
    return 2 * (2 * step + step // 2) + 37


def cotangent(planes, n, seed=5):
    return np.random.default_rng(seed).normal(size=(planes, n)).astype(np.float32)


def run(variant, mode, n):
    """(grad_normal (3, n), grad_weight (K,)) of the 5-frame sequence over n fixed normals."""
    parent = ss.SunskyEmitter(base_dict(), variant)
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    seq.prepare_irradiance(*SIZES[mode], wavelengths=LAMBDAS if variant == "spectral" else None)
    seq.prepare_irradiance_grad()
    planes = seq.irradiance_info()["n_planes"]
    g = seq.irradiance_vjp(torch.from_numpy(sphere_normals(n, 78)).cuda(), torch.from_numpy(cotangent(planes, n)).cuda())
    torch.cuda.synchronize()
    return g["normals"].cpu().numpy(), g["weights"].cpu().numpy()


def main():
    mode, n, outdir = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    torch.cuda.set_device(0)
    for variant in VARIANTS:
        gn, gw = run(variant, mode, n)
        np.save(os.path.join(outdir, f"{variant}_normals.npy"), gn)
        np.save(os.path.join(outdir, f"{variant}_weights.npy"), gw)
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
