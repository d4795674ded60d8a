"""Worker of tests/test_gpu_sequence_irradiance_horizon_grad.py's child-process tests, and the
calls both sides of them make.

As a program (a fresh child process, so that an environment variable the library reads once or
at prepare time takes effect):
    gpu_sequence_irradiance_horizon_grad_worker.py grid <n> <output directory>
        irradiance_vjp(horizon=) of both variants at a 64 x 256 table, 32 sectors, over n
        receivers; started with SUNSKY_AMD_BLOCKS_PER_CU=1, so that every grid-stride loop takes
        several steps
    gpu_sequence_irradiance_horizon_grad_worker.py cap <n> <output directory>
        the same call at a 16 x 32 table, 8 sectors; started with a lowered workspace bound
saves <variant>_normals.npy, <variant>_weights.npy and <variant>_horizon.npy.  Exit 0 = all saved."""
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
from gpu_sequence_irradiance_worker import sphere_normals  # noqa: E402,F401
from gpu_sequence_irradiance_grad_worker import CAP_FLOATS, cotangent, grid_batch_size  # noqa: E402,F401
from gpu_sequence_irradiance_horizon_worker import profiles  # noqa: E402

VARIANTS = ("rgb", "spectral")
SIZES = {"grid": ((64, 256), 32), "cap": ((16, 32), 8)}
KEYS = ("normals", "weights", "horizon")


def run(variant, mode, n):
    """(grad_normal (3, n), grad_weight (K,), grad_horizon (H, n)) of the 5-frame sequence over n
    fixed normals under n fixed profiles."""
    size, sectors = SIZES[mode]
    parent = ss.SunskyEmitter(base_dict(), variant)
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    seq.prepare_irradiance(*size, wavelengths=LAMBDAS if variant == "spectral" else None)
    seq.prepare_irradiance_grad()
    planes = seq.irradiance_info()["n_planes"]
    g = seq.irradiance_vjp(torch.from_numpy(sphere_normals(n, 78)).cuda(), torch.from_numpy(cotangent(planes, n)).cuda(),
                           horizon=torch.from_numpy(profiles(sectors, n, 79)).cuda())
    torch.cuda.synchronize()
    return tuple(g[k].cpu().numpy() for k in KEYS)


def main():
    mode, n, outdir = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    torch.cuda.set_device(0)
    for variant in VARIANTS:
        for key, a in zip(KEYS, run(variant, mode, n)):
            np.save(os.path.join(outdir, f"{variant}_{key}.npy"), a)
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
