"""Worker of tests/test_gpu_sequence_irradiance_horizon.py's grid test, and the call both sides of
it make.

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every grid
is capped at one workgroup per CU):  gpu_sequence_irradiance_horizon_worker.py <n> <output directory>
runs irradiance under per-receiver and shared horizon profiles for both variants and saves
<variant>.npy.  Exit 0 = all saved."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "mitsuba3-sunsky_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sunsky_amd as ss  # noqa: E402
from gpu_sequence_irradiance_worker import VARIANTS, batch_size, sphere_normals  # noqa: E402,F401
from sequence_cases import LAMBDAS, TURBIDITY, WEIGHTS, base_dict, frame_dirs  # noqa: E402

SECTORS = 8


def profiles(sectors, n, seed):
    """(sectors, n) fp32 horizons, uniform in [-0.2, 1.2]: rows cut mid-cell, some sectors fully
    open, some fully closed."""
    return np.random.default_rng(seed).uniform(-0.2, 1.2, (sectors, n)).astype(np.float32)


def run(variant, n):
    """E (2, P, n) of the 5-frame sequence at a 16 x 32 table over n fixed normals: under n
    per-receiver profiles of 8 sectors, then under the first of them shared."""
    parent = ss.SunskyEmitter(base_dict(), variant)
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    seq.prepare_irradiance(16, 32, wavelengths=LAMBDAS if variant == "spectral" else None)
    nrm = torch.from_numpy(sphere_normals(n, 78)).cuda()
    h = torch.from_numpy(profiles(SECTORS, n, 79)).cuda()
    e = torch.stack([seq.irradiance(nrm, horizon=h), seq.irradiance(nrm, horizon=h[:, 0].contiguous())])
    torch.cuda.synchronize()
    return e.cpu().numpy()


def main():
    n, outdir = int(sys.argv[1]), sys.argv[2]
    torch.cuda.set_device(0)
    for variant in VARIANTS:
        np.save(os.path.join(outdir, f"{variant}.npy"), run(variant, n))
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
