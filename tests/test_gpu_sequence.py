"""Frame sequences on the GPU (sunsky_sequence_eval / _bake_latlong): one launch returns
sum_k w_k eval_k(wi) over K frames of one emitter.  Checked against the GPU's own single
emitters, against the oracle, at every launch shape, through the bake, under graph capture and
as a snapshot that outlives its parent."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import oracle as O
import sunsky_amd as ss
import gpu_sequence_worker as W
from helpers import SUN_SLACK, fp32_sun_input, mask_flip_lanes, max_rel, sun_cone_wo
from sequence_cases import (DAY_TIMES, DAY_TURBIDITY, DAY_WEIGHTS, LAMBDAS, TURBIDITY, WEIGHTS, base_dict, batch_wo,
                            frame_dict, frame_dirs, rotation, to_world_dirs)
from test_bake import compare as bake_compare, grid_dirs

pytestmark = pytest.mark.gpu

VARIANTS = ["rgb", "spectral"]
PRECISIONS = ["fast", "reference"]
EPS = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)


def soa(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def single_eval(em, wi_t, lam, active=None):
    """(C, n) of one emitter: eval (RGB) or the broadcast eval at the sequence's wavelengths."""
    if lam is None:
        return em.eval(ss.SurfaceInteraction3f(wi=wi_t), active=active)
    return em.eval_spectral_broadcast(wi_t, lam, active=active)


@functools.lru_cache(maxsize=None)
def case(variant, precision, rotated, frames):
    """One parent, its K-frame sequence, the direction batch, the sequence's result g and every
    frame's single-emitter result v[k], computed once and shared by the checks (read only)."""
    tw = rotation() if rotated else None
    base = base_dict(**({"to_world": tw} if rotated else {}))
    parent = ss.SunskyEmitter(base, variant, precision=precision)
    if frames == "five":
        dirs, turb, wts = frame_dirs(tw), TURBIDITY, WEIGHTS
        seq = ss.SunskySequence(parent, dirs, turb, wts)
    else:   # one day's hourly suns through from_times (night hours included)
        turb, wts = DAY_TURBIDITY, DAY_WEIGHTS
        seq = ss.SunskySequence.from_times(parent, DAY_TIMES, turbidity=turb, weights=wts)
        m = np.asarray(parent.get_param("to_world"), np.float32)[:3, :3]
        dirs = np.stack([m @ ss.sun_coordinates(*t) for t in DAY_TIMES]).astype(np.float32)
    K = len(turb)
    assert seq.info()["count"] == K and seq.info()["precision"] == precision
    local_suns = [seq.frame(k)["sun_dir_local"] for k in range(K)]
    half_ap = parent.info()["sun_half_aperture"]
    wo_local = batch_wo(local_suns, half_ap)
    wi = -to_world_dirs(wo_local, tw)
    wi_t = soa(wi)
    lam = LAMBDAS if variant == "spectral" else None
    g = host(seq.eval(wi_t, lam))
    singles = [ss.SunskyEmitter(frame_dict(base, dirs[k], turb[k]), variant, precision=precision) for k in range(K)]
    for k, em in enumerate(singles):   # the frame IS that emitter's sun: the same fp32 bits
        np.testing.assert_array_equal(em.info()["sun_dir_local"].astype(np.float32), local_suns[k])
    v = [host(single_eval(em, wi_t, lam)) for em in singles]
    return types.SimpleNamespace(base=base, tw=tw, parent=parent, seq=seq, dirs=dirs, turb=turb, wts=wts, K=K,
                                 local_suns=local_suns, half_ap=half_ap, wo_local=wo_local, wi=wi, wi_t=wi_t, lam=lam,
                                 g=g, singles=singles, v=v)


COMBOS = [(v, p, r) for v in VARIANTS for p in PRECISIONS for r in (False, True)]


@pytest.mark.parametrize("variant,precision,rotated", COMBOS)
def test_one_frame_equals_its_single_emitter(variant, precision, rotated):
    """K = 1, w = 1: the project's 1e-5 relative (max_rel's floor) against em_k on the same
    device, over the batch plus directions that straddle frame k's disc edge (the same fp32
    disc decision); below-horizon and masked lanes exactly 0."""
    c = case(variant, precision, rotated, "five")
    n0 = c.wo_local.shape[0]
    for k in range(c.K):
        edge = sun_cone_wo(256, c.local_suns[k], c.half_ap, seed=300 + k, scale=1.0)
        wo_local = np.concatenate([c.wo_local, edge])
        wi_t = soa(-to_world_dirs(wo_local, c.tw))
        n = wo_local.shape[0]
        mask = torch.from_numpy((np.arange(n) % 2).astype(np.uint8)).cuda()
        seq1 = ss.SunskySequence(c.parent, c.dirs[k:k + 1], [c.turb[k]])
        got, got_m = host(seq1.eval(wi_t, c.lam)), host(seq1.eval(wi_t, c.lam, active=mask))
        ref, ref_m = host(single_eval(c.singles[k], wi_t, c.lam)), host(single_eval(c.singles[k], wi_t, c.lam, mask))
        np.testing.assert_array_equal(ref[:, :n0], c.v[k])
        rel, rel_m = max_rel(got, ref), max_rel(got_m, ref_m)
        print(f"frame {k}: max rel {rel:.3e} (masked {rel_m:.3e}), bitwise equal {np.mean(got == ref):.6f}")
        assert rel <= 1e-5 and rel_m <= 1e-5
        below = wo_local[:, 2] < 0
        assert below.sum() >= 16 and np.all(got[:, below] == 0)
        assert np.all(got_m[:, ::2] == 0) and np.any(got_m[:, 1::2] != 0) == (c.local_suns[k][2] >= 0)
        if c.lam is not None:
            assert np.all(got[c.lam.index(300.0)] == 0)   # a wavelength outside the model


@pytest.mark.parametrize("frames", ["five", "day"])
@pytest.mark.parametrize("variant,precision,rotated", COMBOS)
def test_weighted_sum_of_the_gpus_own_single_emitters(variant, precision, rotated, frames):
    """g against sum_k w_k em_k.eval(wi) added in fp64 on the host.  Per lane and plane
    |g - sum| <= (K + 2) 2^-24 sum_k w_k |v_k| + 1e-5 sum_k w_k max(|v_k|, floor_k): the
    worst case of K fp32 products and K - 1 sequential fp32 adds, plus the 1e-5 bar of each
    frame (floor_k = max_rel's 1e-6 max |v_k|)."""
    c = case(variant, precision, rotated, frames)
    S, A, F = (np.zeros(c.g.shape, np.float64) for _ in range(3))
    for k in range(c.K):
        vk = c.v[k].astype(np.float64)
        floor = 1e-6 * max(np.abs(vk).max(), 1e-30)
        S += c.wts[k] * vk
        A += c.wts[k] * np.abs(vk)
        F += c.wts[k] * np.maximum(np.abs(vk), floor)
    bound = (c.K + 2) * EPS * A + 1e-5 * F
    err = np.abs(c.g.astype(np.float64) - S)
    print(f"K = {c.K}: worst {np.max(err / bound):.3f} x bound, max rel {max_rel(c.g, S):.3e}")
    assert np.all(err <= bound), (np.max(err / bound), int((err > bound).sum()))
    assert np.all(c.g[:, c.wo_local[:, 2] < 0] == 0)
    assert sum(s[2] < 0 for s in c.local_suns) >= (1 if frames == "five" else 2)   # suns below the horizon
    assert 0.0 in c.wts


@pytest.mark.parametrize("variant,precision,rotated", COMBOS)
def test_weighted_sum_against_the_oracle(variant, precision, rotated):
    """The 5-frame result against the CPU oracle's frames: a_k / b_k the fp32 / fp64 oracle of
    frame k.  |g - sum_k w_k r_k| <= sum_k w_k beta_k + (K + 2) 2^-24 sum_k w_k |r_k| with, for
    a lane outside frame k's disc, r_k = a_k and beta_k = 1e-5 max(|a_k|, floor_k) + |a_k - b_k|,
    and inside it r_k = b_k and beta_k = 1e-5 |b_k| + s |a_k - b_k| (s = SUN_SLACK).  No lane
    is left out: the batch holds no mask-flip lane for any frame (asserted)."""
    c = case(variant, precision, rotated, "five")
    n = c.wi.shape[0]
    lam_planes = None if c.lam is None else np.repeat(np.asarray(c.lam, np.float32)[:, None], n, 1)
    R, B, A = (np.zeros(c.g.shape, np.float64) for _ in range(3))
    s = SUN_SLACK[precision]
    discs = 0
    for k in range(c.K):
        d = frame_dict(c.base, c.dirs[k], c.turb[k])
        o32 = O.Oracle(d, variant, "jit", "f32")
        o64 = O.Oracle(fp32_sun_input(d, o32), variant, "jit", "f64")
        a, b = o32.eval(c.wi, lam_planes), o64.eval(c.wi, lam_planes)
        a, b = (a.T.astype(np.float64), b.T) if c.lam is None else (a.astype(np.float64), b)
        assert not mask_flip_lanes(a.T, b.T).any(), f"frame {k}: change the seed"
        inf = o32.info()
        inside = (c.wo_local.astype(np.float64) @ inf["sun_dir_local"] >= inf["cos_cutoff"]) & (c.wo_local[:, 2] >= 0)
        discs += int(inside.sum())
        floor = 1e-6 * max(np.abs(a).max(), 1e-30)
        r = np.where(inside, b, a)
        beta = np.where(inside, 1e-5 * np.abs(b) + s * np.abs(a - b), 1e-5 * np.maximum(np.abs(a), floor) + np.abs(a - b))
        R += c.wts[k] * r
        B += c.wts[k] * beta
        A += c.wts[k] * np.abs(r)
    assert discs >= 64 * 4   # every frame above the horizon has its disc lanes
    bound = B + (c.K + 2) * EPS * A
    err = np.abs(c.g.astype(np.float64) - R)
    print(f"worst {np.max(err / np.maximum(bound, 1e-300)):.3f} x bound over {n} lanes, {discs} disc (lane, frame) pairs")
    assert np.all(err <= bound), (np.max(err / np.maximum(bound, 1e-300)), int((err > bound).sum()))


@pytest.mark.parametrize("variant,precision,rotated", COMBOS)
def test_launch_shapes_are_bitwise_the_full_run(variant, precision, rotated):
    """n in {1, 63, 257, 1025}, with and without a mask of alternating bytes: each lane's bits
    are those of the full run's lane (what a direction computes depends on nothing else)."""
    c = case(variant, precision, rotated, "five")
    n_all = c.wi.shape[0]
    mask = torch.from_numpy((np.arange(n_all) % 2).astype(np.uint8)).cuda()
    full_m = host(c.seq.eval(c.wi_t, c.lam, active=mask))
    assert np.all(full_m[:, ::2] == 0)
    np.testing.assert_array_equal(full_m[:, 1::2], c.g[:, 1::2])
    for n in (1, 63, 257, 1025):
        for lo in (0, 1):   # two windows of the batch: a lane's bits do not depend on its index
            wi_n = c.wi_t[:, lo:lo + n].contiguous()
            np.testing.assert_array_equal(host(c.seq.eval(wi_n, c.lam)), c.g[:, lo:lo + n])
            np.testing.assert_array_equal(host(c.seq.eval(wi_n, c.lam, active=mask[lo:lo + n].clone())),
                                          full_m[:, lo:lo + n])
    # strided output planes
    out = torch.full((c.g.shape[0], n_all + 5), -1.0, device="cuda")
    c.seq.eval(c.wi_t, c.lam, out=out[:, :n_all])
    np.testing.assert_array_equal(host(out)[:, :n_all], c.g)
    assert np.all(host(out)[:, n_all:] == -1.0)


def test_a_grid_smaller_than_the_work_is_bitwise_the_default_grid(tmp_path):
    """A child process with SUNSKY_AMD_BLOCKS_PER_CU=1 walks the grid-stride loop two to three
    times per lane; this process makes the same calls at the default grid (one step)."""
    n = W.batch_size()
    env = dict(os.environ, SUNSKY_AMD_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, W.__file__, str(n), str(tmp_path)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"worker exit {r.returncode}:\n{r.stdout[-4000:]}"
    for variant, precision in W.COMBOS:
        child = np.load(tmp_path / f"{variant}_{precision}.npz")["g"]
        mine = W.run(variant, precision, n)
        assert child.shape == mine.shape and np.any(mine != 0)
        np.testing.assert_array_equal(child, mine)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_identity_code_object_gives_the_general_ones_bits(variant, precision, monkeypatch):
    """A sequence over an identity to_world launches the identity code object;
    SUNSKY_AMD_GENERAL_XFORM=1 forces the general one: the same bits, eval and bake."""
    c = case(variant, precision, False, "five")
    bake = host(c.seq.bake_latlong(37, 13, wavelengths=c.lam))
    monkeypatch.setenv("SUNSKY_AMD_GENERAL_XFORM", "1")
    np.testing.assert_array_equal(host(c.seq.eval(c.wi_t, c.lam)), c.g)
    np.testing.assert_array_equal(host(c.seq.bake_latlong(37, 13, wavelengths=c.lam)), bake)


@pytest.mark.parametrize("size", [(37, 13), (128, 64)])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bake_matches_sequence_eval(variant, size, rotated, precision):
    """The lat-long bake of the weighted sum against sequence.eval of host-generated grid
    directions, tests/test_bake.py's bar: 1e-4 relative away from +-2 degrees of the horizon,
    exact 0 below (identity to_world; a rotated one has no flat horizon in the image, so the
    comparison there is 1e-4 where the local direction is 2 degrees clear of it)."""
    c = case(variant, precision, rotated, "five")
    w, h = size
    img = host(c.seq.bake_latlong(w, h, wavelengths=c.lam)).reshape(-1, w * h)
    dirs, theta = grid_dirs(w, h)
    ref = host(c.seq.eval(torch.from_numpy(-dirs).cuda(), c.lam))
    assert np.any(img != 0)
    if not rotated:
        bake_compare(img, ref, theta)
    else:
        local = dirs.T.astype(np.float64) @ np.asarray(c.tw, np.float64)[:3, :3]   # R^-1 d = R^T d
        keep = np.abs(local[:, 2]) > np.sin(np.radians(2))
        b, r = img[:, keep].astype(np.float64), ref[:, keep].astype(np.float64)
        assert (np.abs(b - r) / np.maximum(np.abs(r), 1e-6 * np.abs(r).max())).max() < 1e-4
        assert np.all(img[:, local[:, 2] < -np.sin(np.radians(2))] == 0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_sequence_eval_replays_bitwise_from_a_graph(variant):
    """sequence.eval captured once on a side stream and replayed twice: its output equals the
    direct call bit for bit; nothing is allocated between capture and replay."""
    c = case(variant, "fast", False, "five")
    out = torch.zeros(c.g.shape, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.seq.eval(c.wi_t, c.lam, out=out)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c.seq.eval(c.wi_t, c.lam, out=out)
    allocated = torch.cuda.memory_allocated()
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), c.g)
    assert torch.cuda.memory_allocated() == allocated
    direct = host(c.seq.eval(c.wi_t, c.lam))
    np.testing.assert_array_equal(direct, c.g)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_sequence_is_a_snapshot(variant):
    """get_frame of the device sequence equals the host-only sequence's records bit for bit;
    the sequence evaluates the same after its parent was updated and after it was destroyed."""
    tw = rotation()
    base = base_dict(to_world=tw)
    parent = ss.SunskyEmitter(base, variant)
    dirs = frame_dirs(tw)
    seq = ss.SunskySequence(parent, dirs, TURBIDITY, WEIGHTS)
    host_seq = ss.SunskySequence(ss.SunskyEmitter(base, variant, device="host"), dirs, TURBIDITY, WEIGHTS)
    for k in range(5):
        fd, fh = seq.frame(k), host_seq.frame(k)
        for key in ("sun_dir_local", "sky_params", "sky_radiance"):
            np.testing.assert_array_equal(fd[key], fh[key])
        assert fd["weight"] == fh["weight"] and fd["turbidity"] == fh["turbidity"]
    c = case(variant, "fast", True, "five")
    np.testing.assert_array_equal(host(seq.eval(c.wi_t, c.lam)), c.g)
    p = parent.traverse()
    p["turbidity"] = 8.0
    p["albedo"] = 0.7
    p["sun_direction"] = [0.3, 0.1, 0.6]
    p.update()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(seq.eval(c.wi_t, c.lam)), c.g)
    del p, parent
    np.testing.assert_array_equal(host(seq.eval(c.wi_t, c.lam)), c.g)
