"""Per-frame gradients of a frame sequence on the GPU (sunsky_sequence_eval_vjp), the in-place
update and the autograd bridge.  The reference is the GPU's own single emitters (eval and
eval_jvp, themselves held to finite differences elsewhere), never the sequence's kernels: for
frame k and component c the term of ray i and plane p is r = em_k.eval (weight),
w_k em_k.eval_jvp("turbidity", [1]) or w_k em_k.eval_jvp("sun_direction", (I - s^ s^T) e_a / |s|),
and with S = sum d_out r, A = sum |d_out r|, F = sum |d_out| max(|r|, 1e-6 max |r|) in fp64
    |g - S| <= (m + 2) 2^-24 A + 1e-5 F
for every frame and component, m the longest chain of fp32 additions of the documented
reduction at the launch's geometry (sequence_grad_reference.chain_length)."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import sunsky_amd as ss
import gpu_sequence_grad_worker as W
from sequence_cases import (DAY_TIMES, DAY_TURBIDITY, DAY_WEIGHTS, LAMBDAS, TURBIDITY, WEIGHTS, base_dict, batch_wo,
                            frame_dict, frame_dirs, rotation, to_world_dirs)
from sequence_grad_reference import chain_length, check, frame_terms, grad_array, host, soa, sums, sun_axis_tangents

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
PRECISIONS = ["fast", "reference"]
FRAMES = ["one", "five", "day", "k130"]
REPEATS = {"k130": 26, "k515": 103}   # the five frames repeated: 515 > 512 keeps the waves' rows in the workspace
COMBOS = [(v, p, r) for v in VARIANTS for p in PRECISIONS for r in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def planes_of(variant):
    return len(LAMBDAS) if variant == "spectral" else 3


def frames_of(parent, tw, frames):
    """(world directions, turbidities, weights) of the unique frames of a case."""
    if frames == "one":
        return frame_dirs(tw)[1:2], [TURBIDITY[1]], [1.0]
    if frames == "day":
        m = np.asarray(parent.get_param("to_world"), np.float32)[:3, :3]
        return np.stack([m @ ss.sun_coordinates(*t) for t in DAY_TIMES]).astype(np.float32), DAY_TURBIDITY, DAY_WEIGHTS
    return frame_dirs(tw), TURBIDITY, WEIGHTS


@functools.lru_cache(maxsize=None)
def reference(variant, rotated, frames):
    """The unique frames of a case, the direction batch and every frame's 5 reference terms from
    its reference-precision single emitter, computed once and shared (read only)."""
    tw = rotation() if rotated else None
    base = base_dict(**({"to_world": tw} if rotated else {}))
    parent = ss.SunskyEmitter(base, variant, precision="reference")
    dirs, turb, wts = frames_of(parent, tw, "five" if frames in REPEATS else frames)
    probe = ss.SunskySequence(parent, dirs, turb, wts)
    local_suns = [probe.frame(k)["sun_dir_local"] for k in range(len(turb))]
    half_ap = parent.info()["sun_half_aperture"]
    wo_local = batch_wo(local_suns, half_ap)
    wi_t = soa(-to_world_dirs(wo_local, tw))
    lam = LAMBDAS if variant == "spectral" else None
    singles = [ss.SunskyEmitter(frame_dict(base, dirs[k], turb[k]), variant, precision="reference") for k in range(len(turb))]
    terms = [frame_terms(singles[k], dirs[k], wts[k], wi_t, lam) for k in range(len(turb))]
    n = wi_t.shape[1]
    rng = np.random.default_rng(11)
    d_outs = {"normal": rng.standard_normal((planes_of(variant), n)).astype(np.float32),
              "ones": np.ones((planes_of(variant), n), np.float32)}
    return types.SimpleNamespace(base=base, tw=tw, dirs=dirs, turb=list(turb), wts=list(wts), local_suns=local_suns,
                                 half_ap=half_ap, wo_local=wo_local, wi_t=wi_t, lam=lam, singles=singles, terms=terms,
                                 n=n, d_outs=d_outs, rep=REPEATS.get(frames, 1))


@functools.lru_cache(maxsize=None)
def sequence(variant, precision, rotated, frames):
    """The case's sequence, created at `precision`, gradients prepared."""
    r = reference(variant, rotated, frames)
    parent = ss.SunskyEmitter(r.base, variant, precision=precision)
    seq = ss.SunskySequence(parent, np.tile(r.dirs, (r.rep, 1)), r.turb * r.rep, r.wts * r.rep)
    assert seq.info()["precision"] == precision and len(seq) == len(r.turb) * r.rep
    seq.prepare_grad()
    return seq


def reference_sums(r, d_out, lanes=None):
    """S, A, F (K, 5) of the case (the repeats tiled) over all lanes or the lanes given."""
    terms = r.terms if lanes is None else [[t[:, lanes] for t in f] for f in r.terms]
    d = d_out if lanes is None else d_out[:, lanes]
    return tuple(np.tile(x, (r.rep, 1)) for x in sums(terms, d))


@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("variant,precision,rotated", COMBOS)
def test_gradients_against_the_gpus_own_single_emitters(variant, precision, rotated, frames):
    """Every frame and component within the bound, for a normal and an all-ones cotangent; the
    invalid 300 nm plane adds nothing (its reference terms are 0)."""
    r, seq = reference(variant, rotated, frames), sequence(variant, precision, rotated, frames)
    m = chain_length(r.n, len(seq), planes_of(variant))
    for kind, d_out in r.d_outs.items():
        g = grad_array(seq.eval_vjp(r.wi_t, torch.from_numpy(d_out).cuda(), r.lam))
        check(g, *reference_sums(r, d_out), m, f"{variant} {precision} rotated={rotated} K={len(seq)} d_out {kind}")
        assert np.any(g != 0)
    if r.lam is not None:
        assert all(np.all(t[r.lam.index(300.0)] == 0) for f in r.terms for t in f)


@pytest.mark.parametrize("variant", VARIANTS)
def test_more_frames_than_the_lds_rows_hold(variant):
    """K = 515 > 512: the waves keep their rows in the workspace, not in LDS."""
    test_gradients_against_the_gpus_own_single_emitters(variant, "fast", False, "k515")


@pytest.mark.parametrize("variant,rotated", [(v, r) for v in VARIANTS for r in (False, True)])
def test_one_frame_against_the_single_emitters_eval_vjp(variant, rotated):
    """K = 1, w = 1: grad_turbidity is the single emitter's eval_vjp turbidity entry and
    grad_sun_dir its sun_direction gradient through the normalisation, (I - s^ s^T) / |s| in fp64
    on the host, within the same bound."""
    r, seq = reference(variant, rotated, "one"), sequence(variant, "reference", rotated, "one")
    m = chain_length(r.n, 1, planes_of(variant))
    d_out = r.d_outs["normal"]
    d_t = torch.from_numpy(d_out).cuda()
    g = grad_array(seq.eval_vjp(r.wi_t, d_t, r.lam))
    wl = None if r.lam is None else torch.tensor(r.lam, device="cuda")[:, None].expand(-1, r.n).contiguous()
    _, view = r.singles[0].eval_vjp(ss.SurfaceInteraction3f(wi=r.wi_t, wavelengths=wl), d_t)
    gs = host(view["sun_direction"]).astype(np.float64)
    proj = np.stack(sun_axis_tangents(r.dirs[0])).astype(np.float64) @ gs
    mine = np.concatenate([[float(host(view["turbidity"]))], proj])
    S, A, F = reference_sums(r, d_out)
    check(np.concatenate([[S[0, 0]], mine])[None, :], S, A, F, m, f"{variant} rotated={rotated}: the emitter's eval_vjp")
    check(g, S, A, F, m, f"{variant} rotated={rotated}: K = 1")


@pytest.mark.parametrize("variant,rotated", [(v, r) for v in VARIANTS for r in (False, True)])
def test_structure_of_the_gradient(variant, rotated):
    """The w = 0 frame: zero T and s gradients, a non-zero weight gradient.  The sun below the
    horizon: all zeros.  A masked call equals the call on the compacted active rays within the
    bound.  A batch entirely below the horizon: exact zeros."""
    r, seq = reference(variant, rotated, "five"), sequence(variant, "fast", rotated, "five")
    d_out = r.d_outs["normal"]
    d_t = torch.from_numpy(d_out).cuda()
    g = grad_array(seq.eval_vjp(r.wi_t, d_t, r.lam))
    zero_w, below = r.wts.index(0.0), 4
    assert r.local_suns[below][2] < 0
    assert np.all(g[zero_w, 1:] == 0) and g[zero_w, 0] != 0
    assert np.all(g[below] == 0)
    keep = np.random.default_rng(5).random(r.n) < 0.6
    mask = torch.from_numpy(keep.astype(np.uint8)).cuda()
    gm = grad_array(seq.eval_vjp(r.wi_t, d_t, r.lam, active=mask))
    lanes = np.flatnonzero(keep)
    gc = grad_array(seq.eval_vjp(r.wi_t[:, lanes].contiguous(), d_t[:, lanes].contiguous(), r.lam))
    S, A, F = reference_sums(r, d_out, lanes)
    check(gm, S, A, F, chain_length(r.n, 5, planes_of(variant)), f"{variant} rotated={rotated}: masked")
    check(gc, S, A, F, chain_length(len(lanes), 5, planes_of(variant)), f"{variant} rotated={rotated}: compacted")
    low = np.flatnonzero(r.wo_local[:, 2] < 0)
    assert len(low) >= 16
    gl = grad_array(seq.eval_vjp(r.wi_t[:, low].contiguous(), d_t[:, low].contiguous(), r.lam))
    assert np.all(gl == 0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_accumulation_null_outputs_and_determinism(variant):
    """A second call into the same buffers gives exactly twice the first; with an output left
    out the other two are unchanged bit for bit; two runs are bit equal."""
    r, seq = reference(variant, False, "five"), sequence(variant, "fast", False, "five")
    d_t = torch.from_numpy(r.d_outs["normal"]).cuda()
    first = seq.eval_vjp(r.wi_t, d_t, r.lam)
    once = {k: host(v).copy() for k, v in first.items()}
    again = seq.eval_vjp(r.wi_t, d_t, r.lam)
    for k in once:
        np.testing.assert_array_equal(host(again[k]), once[k])
    seq.eval_vjp(r.wi_t, d_t, r.lam, grad=first)
    for k in once:
        np.testing.assert_array_equal(host(first[k]), 2 * once[k])
    for left_out in once:
        grad = {k: (None if k == left_out else torch.zeros_like(first[k])) for k in once}
        seq.eval_vjp(r.wi_t, d_t, r.lam, grad=grad)
        for k in once:
            if k != left_out:
                np.testing.assert_array_equal(host(grad[k]), once[k])
    assert seq.eval_vjp(r.wi_t[:, :0].contiguous(), d_t[:, :0].contiguous(), r.lam)["weights"].abs().sum() == 0   # n == 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_launch_shapes(variant):
    """n in {1, 63, 64, 65, 255, 257, 1025}: a wave with one lane, one short of / exactly / one
    past a wave, a workgroup boundary on both sides, several workgroups with a ragged tail; the
    odd full batch (n % 4 != 0) is the case above."""
    r, seq = reference(variant, True, "five"), sequence(variant, "fast", True, "five")
    d_out = r.d_outs["normal"]
    assert r.n % 2 == 1 and r.n % 4 != 0
    for n in (1, 63, 64, 65, 255, 257, 1025):
        lanes = np.arange(n) + 3
        g = grad_array(seq.eval_vjp(r.wi_t[:, lanes].contiguous(), torch.from_numpy(d_out[:, lanes]).cuda(), r.lam))
        check(g, *reference_sums(r, d_out, lanes), chain_length(n, 5, planes_of(variant)), f"{variant} n = {n}")


def test_a_capped_grid_takes_three_trips(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 walks the grid-stride loop two to three
    times per workgroup (its rows are added to, not only stored); the reference terms come from
    this process's single emitters."""
    n = W.batch_size()
    env = dict(os.environ, SUNSKY_AMD_BLOCKS_PER_CU="1")
    p = subprocess.run([sys.executable, W.__file__, str(n), str(tmp_path)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, f"worker exit {p.returncode}:\n{p.stdout[-4000:]}"
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    for variant in W.VARIANTS:
        parent, seq, wi, d_out = W.inputs(variant, n)
        lam = LAMBDAS if variant == "spectral" else None
        dirs = frame_dirs()
        terms = [frame_terms(ss.SunskyEmitter(frame_dict(base_dict(), dirs[k], TURBIDITY[k]), variant, precision="reference"),
                             dirs[k], WEIGHTS[k], wi, lam) for k in range(5)]
        S, A, F = sums(terms, host(d_out))
        m = chain_length(n, 5, planes_of(variant), blocks_per_cu=1, cu_count=cu)
        assert -(-n // (cu * 256)) == 3
        check(np.load(tmp_path / f"{variant}.npz")["g"], S, A, F, m, f"{variant}: one workgroup per CU, n = {n}")
        check(grad_array(seq.eval_vjp(wi, d_out, lam)), S, A, F, chain_length(n, 5, planes_of(variant)),
              f"{variant}: default grid, n = {n}")


@pytest.mark.parametrize("variant", VARIANTS)
def test_eval_vjp_replays_bitwise_from_a_graph(variant):
    """One captured eval_vjp replayed twice into zeroed buffers equals the eager result bit for
    bit; nothing is allocated between capture and replay."""
    r, seq = reference(variant, False, "five"), sequence(variant, "fast", False, "five")
    d_t = torch.from_numpy(r.d_outs["normal"]).cuda()
    eager = {k: host(v).copy() for k, v in seq.eval_vjp(r.wi_t, d_t, r.lam).items()}
    grad = {k: torch.zeros_like(torch.from_numpy(v)).cuda() for k, v in eager.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seq.eval_vjp(r.wi_t, d_t, r.lam, grad=grad)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seq.eval_vjp(r.wi_t, d_t, r.lam, grad=grad)
    allocated = torch.cuda.memory_allocated()
    for _ in range(2):
        for v in grad.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            np.testing.assert_array_equal(grad[k].cpu().numpy(), eager[k])
    assert torch.cuda.memory_allocated() == allocated


@pytest.mark.parametrize("variant", VARIANTS)
def test_update_equals_a_new_sequence(variant):
    """update followed by eval, eval_vjp and frame_tangent equals a newly created sequence bit
    for bit (the parent destroyed in between: the sequence restages from its own copies); the
    sampling distribution is dropped until prepare_sampling."""
    r = reference(variant, True, "five")
    parent = ss.SunskyEmitter(r.base, variant)
    seq = ss.SunskySequence(parent, r.dirs[::-1].copy(), 3.0, None)
    seq.prepare_grad()
    seq.prepare_sampling(8, 16)
    fresh = ss.SunskySequence(parent, r.dirs, r.turb, r.wts)
    fresh.prepare_grad()
    del parent
    seq.update(r.dirs, r.turb, r.wts)
    with pytest.raises(ValueError, match="prepare_sampling"):
        seq.sampling_info()
    d_t = torch.from_numpy(r.d_outs["normal"]).cuda()
    np.testing.assert_array_equal(host(seq.eval(r.wi_t, r.lam)), host(fresh.eval(r.wi_t, r.lam)))
    a, b = seq.eval_vjp(r.wi_t, d_t, r.lam), fresh.eval_vjp(r.wi_t, d_t, r.lam)
    for k in a:
        np.testing.assert_array_equal(host(a[k]), host(b[k]))
    for k in range(5):
        fa, fb = seq.frame(k), fresh.frame(k)
        ta, tb = seq.frame_tangent(k), fresh.frame_tangent(k)
        for key in ("sun_dir_local", "sky_params", "sky_radiance"):
            np.testing.assert_array_equal(fa[key], fb[key])
        for key in ta:
            np.testing.assert_array_equal(ta[key], tb[key])
    seq.update(weights=[1.0] * 5)   # a partial update keeps the other arrays
    assert [seq.frame(k)["turbidity"] for k in range(5)] == [np.float32(t) for t in r.turb]
    seq.prepare_sampling(8, 16)
    assert seq.sampling_info()["n_z"] == 8


@pytest.mark.parametrize("variant", VARIANTS)
def test_frame_tangents_are_the_device_emitters(variant):
    """dsky_turbidity of the device-staged record is the device-staged tangent table of the
    frame's single emitter, bit for bit."""
    r, seq = reference(variant, True, "five"), sequence(variant, "fast", True, "five")
    for k in range(5):
        ref = r.singles[k].tangent_tables("turbidity", [1.0], on_device=True)["dsky"]
        np.testing.assert_array_equal(seq.frame_tangent(k)["dsky_turbidity"], ref)


@pytest.mark.parametrize("variant", VARIANTS)
def test_autograd_bridge(variant):
    """sequence_eval's value is seq.eval's bits, the gradients of (d_out * y).sum() are
    eval_vjp's bits for exactly the tensors passed, and one small gradient step on the weights
    and turbidities towards a target made from known parameters lowers the squared error."""
    r = reference(variant, False, "five")
    parent = ss.SunskyEmitter(r.base, variant)
    seq = ss.SunskySequence(parent, r.dirs, r.turb, r.wts)
    d_t = torch.from_numpy(r.d_outs["normal"]).cuda()
    w = torch.tensor(r.wts, requires_grad=True)
    T = torch.tensor(r.turb, device="cuda", requires_grad=True)
    s = torch.tensor(r.dirs, device="cuda", requires_grad=True)
    y = ss.sequence_eval(seq, r.wi_t, w, T, s, wavelengths=r.lam)
    np.testing.assert_array_equal(host(y.detach()), host(seq.eval(r.wi_t, r.lam)))
    (d_t * y).sum().backward()
    g = seq.eval_vjp(r.wi_t, d_t, r.lam)
    np.testing.assert_array_equal(w.grad.numpy(), host(g["weights"]))
    np.testing.assert_array_equal(host(T.grad), host(g["turbidity"]))
    np.testing.assert_array_equal(host(s.grad), host(g["sun_directions"]))
    w2 = torch.tensor(r.wts, device="cuda", requires_grad=True)
    y2 = ss.sequence_eval(seq, r.wi_t, weights=w2, wavelengths=r.lam)
    (d_t * y2).sum().backward()
    np.testing.assert_array_equal(host(w2.grad), host(g["weights"]))
    # a fit: the target from the known parameters, the start a little off in w and T
    target = seq.eval(r.wi_t, r.lam).clone()
    w0 = torch.tensor([x * 1.1 + 0.05 for x in r.wts], device="cuda", requires_grad=True)
    T0 = torch.tensor([min(max(t * 1.05, 1.0), 9.5) for t in r.turb], device="cuda", requires_grad=True)
    loss0 = ((ss.sequence_eval(seq, r.wi_t, w0, T0, wavelengths=r.lam) - target) ** 2).sum()
    loss0.backward()
    with torch.no_grad():
        # a step along -grad short enough for the linear model to hold: 1e-3 of the parameters' norm
        gn = torch.sqrt((w0.grad ** 2).sum() + (T0.grad ** 2).sum())
        step = 1e-3 * torch.sqrt((w0 ** 2).sum() + (T0 ** 2).sum()) / gn
        w1, T1 = (w0 - step * w0.grad).clamp(min=0), (T0 - step * T0.grad).clamp(1, 10)
        loss1 = ((ss.sequence_eval(seq, r.wi_t, w1, T1, wavelengths=r.lam) - target) ** 2).sum()
    loss0, loss1 = float(loss0.detach()), float(loss1)
    print(f"{variant}: loss {loss0:.6e} -> {loss1:.6e}")
    assert loss1 < loss0
