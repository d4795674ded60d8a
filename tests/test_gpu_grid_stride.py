"""More than one grid-stride step per lane.  Every batch kernel is a grid-stride loop over a grid
capped at a number of workgroups per CU; at the default caps only a batch beyond ~16.8M
directions makes a lane take a second step, so no other test walks these kernels' loops twice,
nor takes the 11-node broadcast kernel with its dynamic-LDS occupancy cap (which engages only
then).  (The worker leaves out the six direct-lighting kernels, sunsky_sample_wavelengths_{rgb,
spec} and sunsky_bake_latlong_{rgb,spec}: tests/test_gpu_direct_shapes.py walks their loops two
to three times in the same way, with gpu_direct_worker.py; the sequence kernels have capped-grid
tests of their own.) A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 (one workgroup per CU) runs
a batch of ~655k directions, one in eight of them inside the sun disc (the disc lanes' second
pass of the broadcast kernels).  eval, eval_direction, pdf_direction and eval_spectral_broadcast
get 16-byte-aligned planes through the C ABI (gpu_grid_stride_worker.py), so each call is a
4-directions-per-lane body of two to three steps per lane and a 3-element scalar tail; the
sampling kernels take 3 to 10 steps.  This process makes the same calls at the default grid (one
step per lane).  Every output must be the same bit for bit: what a direction computes does not
depend on the grid.

The grid itself cannot be observed from here: the test relies on the override being honoured
(it is read in one place, grid_for of csrc/sunsky_launch.cpp, once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpu_grid_stride_worker as W

pytestmark = pytest.mark.gpu


def test_outputs_do_not_depend_on_the_grid(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    n = W.batch_size()
    env = dict(os.environ, SUNSKY_AMD_BLOCKS_PER_CU="1")
    # a child that fails or hangs fails the test here, before any GPU work of this process
    r = subprocess.run([sys.executable, W.__file__, str(n), str(tmp_path)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    inp = W.inputs(n)
    for variant, precision in W.COMBOS:
        path = tmp_path / f"{variant}_{precision}.npz"
        with np.load(path) as stepped:
            single = W.run(variant, precision, inp)
            assert sorted(stepped.files) == sorted(single)
            for name, a in single.items():
                b = stepped[name]
                assert a.shape == b.shape, (variant, precision, name, a.shape, b.shape)
                same = (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))
                assert bool(same.all()), f"{variant} {precision} {name}: {int((~same).sum())} of {same.size} values differ"
        path.unlink()
