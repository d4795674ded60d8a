"""Worker of tests/test_gpu_sequence_irradiance.py's grid test, and the call both sides of it make.

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every
grid is capped at one workgroup per CU):  gpu_sequence_irradiance_worker.py <n> <output directory>
runs irradiance for both variants and saves <variant>.npy.  Exit 0 = all saved."""
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

VARIANTS = ("rgb", "spectral")


def batch_size():
    """Two and a half grid-stride steps of a one-receiver-per-lane kernel at one workgroup per CU,
    plus an odd remainder: some lanes take three steps, some two."""
    step = torch.cuda.get_device_properties(0).multi_processor_count * 256
    return 2 * step + step // 2 + 37


def sphere_normals(n, seed):
    """(3, n) fp32 unit vectors, uniform on the whole sphere."""
    v = np.random.default_rng(seed).normal(size=(3, n))
    return (v / np.linalg.norm(v, axis=0)).astype(np.float32)


def run(variant, n):
    """E (P, n) of the 5-frame sequence at a 16 x 32 table over n fixed normals."""
    parent = ss.SunskyEmitter(base_dict(), variant)
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    seq.prepare_irradiance(16, 32, wavelengths=LAMBDAS if variant == "spectral" else None)
    e = seq.irradiance(torch.from_numpy(sphere_normals(n, 78)).cuda())
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
