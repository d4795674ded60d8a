"""Worker of tests/test_gpu_sequence_irradiance_series.py's grid test, and the call both sides of
it make.

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every grid
is capped at one workgroup per CU):  gpu_sequence_irradiance_series_worker.py <output directory>
runs the irradiance series with an open horizon and under per-receiver profiles for both variants
and saves <variant>.npy.  Exit 0 = all saved."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "mitsuba3-sunsky_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sunsky_amd as ss  # noqa: E402
from sunsky_amd import _capi  # noqa: E402
from gpu_sequence_irradiance_horizon_worker import profiles  # noqa: E402
from gpu_sequence_irradiance_worker import VARIANTS, sphere_normals  # noqa: E402,F401
from sequence_cases import base_dict  # noqa: E402

N = 4099
SIZE = (3, 20)
SECTORS = 4
LAMBDAS_32 = [float(x) for x in np.linspace(330.0, 715.0, 31)] + [300.0]


def work_items(frames, planes, n=N):
    """The series kernel's work items: (tile of 256 receiver pairs, group of G frames)."""
    g = _capi.seq_irr_series_group(planes)
    return -(-((n + 1) // 2) // 256) * -(-frames // g)


def frame_count(variant):
    """Frames for more than two grid-stride steps at one workgroup per CU over N receivers: the
    work items are (tile, group), so a small n needs many groups."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    planes = 3 if variant == "rgb" else len(LAMBDAS_32)
    g = _capi.seq_irr_series_group(planes)
    tiles = -(-((N + 1) // 2) // 256)
    groups = 2 * cus // tiles + 3
    return groups * g - 1          # the last group is not full


def suns(count):
    """count sun directions: elevations from -10 to 80 degrees and back, azimuths all around."""
    t = np.arange(count) / max(count - 1, 1)
    e = np.deg2rad(-10.0 + 90.0 * np.abs(np.sin(3.0 * np.pi * t)))
    a = 2.0 * np.pi * 7.0 * t
    return np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], 1).astype(np.float32)


def run(variant):
    """The series (2, K, P, N) of a many-frame sequence at a 3 x 20 table over N fixed normals: with
    an open horizon, then under N per-receiver profiles of 4 sectors."""
    count = frame_count(variant)
    parent = ss.SunskyEmitter(base_dict(), variant)
    turb = [1.0 + 9.0 * ((7 * k) % 31) / 30.0 for k in range(count)]
    seq = ss.SunskySequence(parent, suns(count), turb, None)
    seq.prepare_irradiance(*SIZE, wavelengths=LAMBDAS_32 if variant == "spectral" else None)
    seq.prepare_irradiance_series()
    nrm = torch.from_numpy(sphere_normals(N, 78)).cuda()
    h = torch.from_numpy(profiles(SECTORS, N, 79)).cuda()
    e = torch.stack([seq.irradiance_series(nrm), seq.irradiance_series(nrm, horizon=h)])
    torch.cuda.synchronize()
    return e.cpu().numpy()


def main():
    outdir = sys.argv[1]
    torch.cuda.set_device(0)
    for variant in VARIANTS:
        np.save(os.path.join(outdir, f"{variant}.npy"), run(variant))
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
