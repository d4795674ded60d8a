"""Growth of a handle's ordered scratch buffer on a live handle.  The angle tables of
bake_latlong (emitter and sequence) and the per-workgroup partials of eval_vjp are per-handle
device buffers that the previous call's kernels, queued on any stream, may still be reading
when the next call needs them larger: the call orders its stream after the previous one, and
the host waits for it before the old block is freed.  Each test makes a small call, then a
larger one on a second stream with no host synchronisation in between, and holds both results
bit for bit to what a fresh handle returns for that single call: a block freed or rewritten
under the queued reader, or a second call reading stale tables, changes bits.

eval_vjp repeats bit for bit from call to call (its partials are reduced by one workgroup in
a fixed order, no atomics), so the gradients are compared bitwise too."""
import numpy as np
import pytest
import torch

import sunsky_amd as ss
from helpers import angles_dict, hemisphere_wo

pytestmark = pytest.mark.gpu

SCENE = angles_dict(3.0, 1.0, 0.9, 0.2, 1.0, 1.0)   # sun_direction given: all 5 VJP bases
SMALL, LARGE = (8, 4), (64, 32)   # (width, height): 24 and 192 table floats
SUNS = np.array([[0.3, 0.2, 0.8], [-0.5, 0.1, 0.4]], np.float32)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def _emitter():
    return ss.load_dict(SCENE)   # RGB


def _sequence():
    return ss.SunskySequence(_emitter(), SUNS, turbidity=[2.5, 4.0], weights=[1.0, 0.5])


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _small_then_large(first, second):
    """first() on the current stream, second() on another one, no host wait in between."""
    side = torch.cuda.Stream()
    a = first()
    with torch.cuda.stream(side):
        b = second()
    torch.cuda.synchronize()
    return a, b


@pytest.mark.parametrize("make", [_emitter, _sequence], ids=["emitter", "sequence"])
def test_bake_tables_grow_under_a_queued_bake(make):
    live = make()
    small, large = _small_then_large(lambda: live.bake_latlong(*SMALL), lambda: live.bake_latlong(*LARGE))
    for image, size in ((small, SMALL), (large, LARGE)):
        fresh = make().bake_latlong(*size)
        torch.cuda.synchronize()
        assert torch.isfinite(image).all() and float(image.max()) > 0.0
        assert _same_bits(image, fresh), f"bake {size} on a live handle differs from a fresh handle's"


def _vjp_inputs(n):
    wi = torch.from_numpy(np.ascontiguousarray(-hemisphere_wo(n, seed=7).T.astype(np.float32))).cuda()
    cot = torch.from_numpy(np.random.default_rng(11).standard_normal((3, n)).astype(np.float32)).cuda()
    return ss.SurfaceInteraction3f(wi=wi), cot


def test_vjp_partials_grow_under_a_queued_reduce():
    calls = [_vjp_inputs(256), _vjp_inputs(2048)]   # 1 workgroup, then 8
    live = _emitter()
    got = _small_then_large(lambda: live.eval_vjp(*calls[0])[0], lambda: live.eval_vjp(*calls[1])[0])
    for grad, (si, cot) in zip(got, calls):
        fresh = _emitter().eval_vjp(si, cot)[0]
        torch.cuda.synchronize()
        assert torch.isfinite(grad).all() and float(grad.abs().max()) > 0.0
        assert _same_bits(grad, fresh), (grad.cpu().numpy(), fresh.cpu().numpy())
