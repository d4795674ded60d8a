"""Reference of the frame-sequence gradient tests (test_gpu_sequence_grad.py and its worker):
the per-ray, per-plane terms of every frame from the GPU's own single emitters, their fp64
sums against a cotangent, and the length of the fp32 addition chain of sequence.eval_vjp's
documented reduction."""
import numpy as np
import torch

import sunsky_amd as ss
from sunsky_amd import _capi

EPS = 2.0 ** -24
COMPONENTS = ("weights", "turbidity", "sun_x", "sun_y", "sun_z")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def soa(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).cuda()


def sun_axis_tangents(s):
    """(I - s^ s^T) e_a / |s| for a = x, y, z: the tangents of the normalised direction along the
    world axes of the direction as given, fp32 like every tangent the emitter takes."""
    s = np.asarray(s, np.float64)
    length = np.linalg.norm(s)
    u = s / length
    return [((np.eye(3)[a] - u * u[a]) / length).astype(np.float32) for a in range(3)]


def frame_terms(em, sun_dir, weight, wi_t, lam, active=None):
    """The 5 reference terms r[c] (planes, n) fp64 of one frame from its single emitter `em`
    (reference precision): eval for the weight, w eval_jvp("turbidity", [1]) and
    w eval_jvp("sun_direction", (I - s^ s^T) e_a / |s|) for the parameters."""
    n = wi_t.shape[1]
    wl = None if lam is None else torch.tensor(lam, dtype=torch.float32, device="cuda")[:, None].expand(-1, n).contiguous()
    si = ss.SurfaceInteraction3f(wi=wi_t, wavelengths=wl)
    out = [host(em.eval(si, active)).astype(np.float64)]
    out.append(weight * host(em.eval_jvp(si, "turbidity", [1.0], active)[1]).astype(np.float64))
    for tan in sun_axis_tangents(sun_dir):
        out.append(weight * host(em.eval_jvp(si, "sun_direction", tan, active)[1]).astype(np.float64))
    return out


def sums(terms, d_out):
    """S, A, F (K, 5) in fp64 for the terms of K frames against the cotangent d_out (planes, n):
    S = sum d_out r, A = sum |d_out r|, F = sum |d_out| max(|r|, 1e-6 max |r|)."""
    d = np.asarray(d_out, np.float64)
    K = len(terms)
    S, A, F = (np.zeros((K, 5)) for _ in range(3))
    for k, frame in enumerate(terms):
        for c, r in enumerate(frame):
            floor = 1e-6 * np.abs(r).max()
            S[k, c] = (d * r).sum()
            A[k, c] = np.abs(d * r).sum()
            F[k, c] = (np.abs(d) * np.maximum(np.abs(r), floor)).sum()
    return S, A, F


def chain_length(n, count, planes, blocks_per_cu=None, cu_count=None):
    """The longest chain of fp32 additions one of eval_vjp's sums passes through, from the
    documented reduction (include/sunsky_amd.h, csrc/sunsky_kernel_args.h) and the launch
    geometry:
      a lane adds a sky term and at most one disc term per plane (2 planes), folds the
      unit-elevation sum into a sun sum (1) and the gamma part (1);
      the wave adds 64 lanes by 6 shuffle steps;
      lane 0 adds the wave's sum to its row once per grid-stride trip after the first;
      count <= 512: the workgroup adds its 4 waves' rows into one (3), rows = grid; else rows = 4 grid;
      the reduce kernel's lane adds ceil(rows / 64) rows (the first onto 0), the wave 6 more
      steps, and lane 0 adds the total to the output (1).
    grid = min(ceil(n / 256), CUs x workgroups per CU, max(1, workspace // (5 count rows per workgroup)))."""
    if cu_count is None:
        cu_count = torch.cuda.get_device_properties(0).multi_processor_count
    if blocks_per_cu is None:
        blocks_per_cu = _capi.SEQ_GRAD_BLOCKS_PER_CU
    per_group = 1 if count <= _capi.SEQ_GRAD_LDS_FRAMES else 4
    grid = min(-(-n // 256), cu_count * blocks_per_cu, max(1, _capi.SEQ_GRAD_WORKSPACE_FLOATS // (5 * count * per_group)))
    trips = -(-n // (grid * 256))
    rows = grid * per_group
    return 2 * planes + 2 + 6 + (trips - 1) + (3 if per_group == 1 else 0) + -(-rows // 64) + 6 + 1


def grad_array(g):
    """eval_vjp's dict as a (K, 5) fp64 array in COMPONENTS order."""
    return np.concatenate([host(g["weights"])[:, None], host(g["turbidity"])[:, None], host(g["sun_directions"])],
                          axis=1).astype(np.float64)


def check(g, S, A, F, m, what):
    """|g - S| <= (m + 2) 2^-24 A + 1e-5 F for every frame and component; prints the worst ratio."""
    bound = (m + 2) * EPS * A + 1e-5 * F
    err = np.abs(g - S)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    k, c = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"{what}: m = {m}, worst {ratio.max():.3f} x bound (frame {k}, {COMPONENTS[c]})")
    assert np.all(err <= bound), (what, float(ratio.max()), int(k), COMPONENTS[c], float(g[k, c]), float(S[k, c]))
    return float(ratio.max())
