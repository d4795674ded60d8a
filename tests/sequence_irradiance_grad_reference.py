"""numpy restatement of the gradients of a sequence's irradiance (include/sunsky_amd.h,
"gradients of the irradiance") in fp64 over the tables read back from the product:

    grad_normal(r) = M^T g_l(r),  g_l(r) = sum_e a_r[e] dir_e [n_l . dir_e > 0],
                     a_r[e] = sum_p d_out[p, r] term_p[e]      (e: the cells, then the suns)
    grad_weight[k] = omega sum_p sum_ij G_p[i, j] S_k[p, i, j] + sum_p H_p[k] F_k[p]

with A, B and the cell centres as tests/sequence_irradiance_reference.py takes them, the
per-frame sky tables S_k read back as irradiance_table("sky") of a sequence over the same frames
with one-hot weights (fma(1, v, 0) is exact), and F from irradiance_table("sun_flux").  Beside
each value the magnitudes the rounding bounds of tests/test_gpu_sequence_irradiance_grad.py need."""
import numpy as np

import sunsky_amd as ss
from sunsky_amd import _capi
from sequence_irradiance_reference import IrradianceReference

EPS = 2.0 ** -24


def frame_sky_tables(parent, dirs, turbidity, size, lam):
    """(K, P, cells) fp64: frame k's unweighted sky term at the cell centres."""
    K = len(turbidity)
    seq = ss.SunskySequence(parent, dirs, turbidity, [1.0] + [0.0] * (K - 1))
    out = []
    for k in range(K):
        if k:
            seq.update(weights=[1.0 if j == k else 0.0 for j in range(K)])
        seq.prepare_irradiance(*size, wavelengths=lam)
        t = seq.irradiance_table("sky").astype(np.float64)
        out.append(t.reshape(t.shape[0], -1))
    return np.stack(out)


class IrradianceGradReference:
    def __init__(self, seq, sky_frames, to_world=None):
        r = self.r = IrradianceReference(seq)
        self.S = np.asarray(sky_frames, np.float64)                       # (K, P, cells)
        assert self.S.shape == (r.K, r.planes, r.n_z * r.n_phi)
        self.dirs = np.concatenate([r.centres, r.suns])                   # (cells + K, 3)
        self.terms = np.concatenate([r.sky_terms, r.sun_terms], axis=1)   # (P, cells + K)
        # grad_world = (to_local's linear part)^T g_l = R g_l for to_world's rotation R
        self.R = np.eye(3) if to_world is None else np.asarray(to_world, np.float64)[:3, :3]

    # ------------------------------------------------------------ normals
    def normal_grad(self, normals_local, d_out, chunk=256):
        """(grad (3, n), M (3, n), slack (3, n)) in world space for (n, 3) local normals and a
        (P, n) cotangent.  M = sum |terms|; slack = sum |a_r dir| over the records whose fp64
        |n_l . dir| is below 8 2^-24 |n_l|: a step may fall either way there."""
        nl, d = np.asarray(normals_local, np.float64), np.asarray(d_out, np.float64)
        n = nl.shape[0]
        g, M, slack = np.zeros((3, n)), np.zeros((3, n)), np.zeros((3, n))
        absdirs, absterms = np.abs(self.dirs), np.abs(self.terms)
        for lo in range(0, n, chunk):
            sl = slice(lo, lo + chunk)
            dots = nl[sl] @ self.dirs.T                                   # (c, E)
            a = d[:, sl].T @ self.terms
            amag = np.abs(d[:, sl]).T @ absterms
            step = dots > 0
            near = np.abs(dots) < 8 * EPS * np.linalg.norm(nl[sl], axis=1, keepdims=True)
            g[:, sl] = ((a * step) @ self.dirs).T
            M[:, sl] = ((amag * step) @ absdirs).T
            slack[:, sl] = ((np.abs(a) * near) @ absdirs).T
        aR = np.abs(self.R)
        return self.R @ g, aR @ M, aR @ slack

    def normal_bound(self, M, slack):
        """1e-5 M (table rounding) + (n_phi + n_z + K + P + 4) 2^-24 M (the header's depth, and 4
        for the dot product, to_local and its transpose) + slack."""
        r = self.r
        return 1e-5 * M + (r.n_phi + r.n_z + r.K + r.planes + 4) * EPS * M + slack

    # ------------------------------------------------------------ weights
    def adjoint(self, normals_local, d_out, chunk=512):
        """(G (P, cells + K), |G|): the adjoint image of the cotangent and its magnitude."""
        nl, d = np.asarray(normals_local, np.float64), np.asarray(d_out, np.float64)
        G, Gm = np.zeros(self.terms.shape), np.zeros(self.terms.shape)
        for lo in range(0, nl.shape[0], chunk):
            cos = np.maximum(nl[lo:lo + chunk] @ self.dirs.T, 0.0)
            G += d[:, lo:lo + chunk] @ cos
            Gm += np.abs(d[:, lo:lo + chunk]) @ cos
        return G, Gm

    def weight_grad(self, normals_local, d_out):
        """(grad (K,), M (K,)): every frame's dL/dw_k and the sum of the magnitudes of its terms.
        A frame whose sun is below the horizon gets exactly 0."""
        r = self.r
        G, Gm = self.adjoint(normals_local, d_out)
        q = r.n_z * r.n_phi
        gw = r.omega * np.einsum("pe,kpe->k", G[:, :q], self.S) + np.einsum("pk,pk->k", G[:, q:], r.F)
        M = r.omega * np.einsum("pe,kpe->k", Gm[:, :q], np.abs(self.S)) + np.einsum("pk,pk->k", Gm[:, q:], np.abs(r.F))
        night = r.suns[:, 2] < 0
        gw[night] = 0.0
        return gw, M

    def weight_depth(self, n, cap=_capi.SEQ_IRR_GRAD_WORKSPACE_FLOATS):
        """m of the header: 256 + slice_len / 256 + slices + P ceil(Q / 256) + P + 11."""
        r = self.r
        q = r.n_z * r.n_phi
        slices, length = _capi.seq_irr_grad_shape(n, r.planes, q, r.K, cap)
        return 256 + length // 256 + slices + r.planes * -(-q // 256) + r.planes + 11

    def weight_bound(self, M, n, cap=_capi.SEQ_IRR_GRAD_WORKSPACE_FLOATS):
        return (self.weight_depth(n, cap) + 2) * EPS * M + 1e-5 * M
