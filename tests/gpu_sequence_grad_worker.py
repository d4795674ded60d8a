"""Worker of tests/test_gpu_sequence_grad.py's capped-grid test, and the calls both sides make.

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every
grid is capped at one workgroup per CU):  gpu_sequence_grad_worker.py <n> <output directory>
runs sequence.eval_vjp of the 5-frame sequence for both variants and saves <variant>.npz.
Exit 0 = all saved."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "mitsuba3-sunsky_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sunsky_amd as ss  # noqa: E402
from sequence_cases import LAMBDAS, TURBIDITY, WEIGHTS, base_dict, batch_wo, frame_dirs  # noqa: E402
from sequence_grad_reference import grad_array  # noqa: E402

VARIANTS = ("rgb", "spectral")


def batch_size():
    """Two and a half grid-stride trips at one workgroup per CU (plus the batch's odd
    remainder): some workgroups take three trips, some two."""
    step = torch.cuda.get_device_properties(0).multi_processor_count * 256
    return 2 * step + step // 2 + 37 + 5 * 64 + 16


def inputs(variant, n):
    """The parent, the 5-frame sequence (gradients prepared), wi (3, n) and a normal cotangent."""
    parent = ss.SunskyEmitter(base_dict(), variant, precision="reference")
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    seq.prepare_grad()
    suns = [seq.frame(k)["sun_dir_local"] for k in range(5)]
    wo = batch_wo(suns, parent.info()["sun_half_aperture"], n_sky=n - 5 * 64 - 16)
    assert wo.shape[0] == n
    wi = torch.from_numpy(np.ascontiguousarray(-wo.T)).cuda()
    planes = len(LAMBDAS) if variant == "spectral" else 3
    d_out = torch.from_numpy(np.random.default_rng(77).standard_normal((planes, n)).astype(np.float32)).cuda()
    return parent, seq, wi, d_out


def run(variant, n):
    _, seq, wi, d_out = inputs(variant, n)
    return grad_array(seq.eval_vjp(wi, d_out, LAMBDAS if variant == "spectral" else None))


def main():
    n, outdir = int(sys.argv[1]), sys.argv[2]
    torch.cuda.set_device(0)
    for variant in VARIANTS:
        np.savez(os.path.join(outdir, f"{variant}.npz"), g=run(variant, n))
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
