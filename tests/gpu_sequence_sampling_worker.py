"""Worker of tests/test_gpu_sequence_sampling.py's grid test, and the call both sides of it make.

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every
grid is capped at one workgroup per CU):  gpu_sequence_sampling_worker.py <n> <output directory>
runs sample_direction + pdf_direction for every (variant, precision) and saves
<variant>_<precision>.npz.  Exit 0 = all saved."""
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

COMBOS = [(v, p) for v in ("rgb", "spectral") for p in ("fast", "reference")]


def batch_size():
    """Two and a half grid-stride steps of a one-sample-per-lane kernel at one workgroup per CU,
    plus an odd remainder: some lanes take three steps, some two."""
    step = torch.cuda.get_device_properties(0).multi_processor_count * 256
    return 2 * step + step // 2 + 37


def run(variant, precision, n):
    """(d, pdf, weight, pdf_direction(d)) of the 5-frame sequence over n fixed samples."""
    parent = ss.SunskyEmitter(base_dict(), variant, precision=precision)
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    seq.prepare_sampling(16, 32)
    u = torch.from_numpy(np.random.default_rng(77).random((2, n), dtype=np.float32)).cuda()
    ds, w = seq.sample_direction(None, u, LAMBDAS if variant == "spectral" else None)
    p = seq.pdf_direction(None, ds)
    torch.cuda.synchronize()
    return {"d": ds.d.cpu().numpy(), "pdf": ds.pdf.cpu().numpy(), "w": w.cpu().numpy(), "p": p.cpu().numpy()}


def main():
    n, outdir = int(sys.argv[1]), sys.argv[2]
    torch.cuda.set_device(0)
    for variant, precision in COMBOS:
        np.savez(os.path.join(outdir, f"{variant}_{precision}.npz"), **run(variant, precision, n))
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
