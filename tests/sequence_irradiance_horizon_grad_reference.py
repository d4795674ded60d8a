"""numpy restatement of the gradients of a sequence's irradiance under a horizon profile
(include/sunsky_amd.h, "gradients of the irradiance under a horizon profile") in fp64 over the
tables read back from the product.  It builds on HorizonReference (the visible share v and the
suns' visibility) and IrradianceGradReference (the records, the plane folds, the open bounds);
the per-frame sky tables are irradiance_frame_table(k).

    grad_normal(r)   = R sum_e V_r[e] a_r[e] dir_e [n_l . dir_e > 0]
    grad_weight[k]   = omega sum_p sum_ij G_p[i, j] S_k[p, i, j] + sum_p H_p[k] F_k[p]
    grad_horizon[b, r] = -n_z sum_i [0 < t_r[i, b] < 1] sum_{j in b} max(0, n_l . c_ij) a_r[i, j]

with V = v over the cells (exact in fp64 from the fp32 h) and the 0 / 1 visibility over the suns,
G and H the adjoint image taken with V.  For the horizon gradient t = i + 1 - h n_z is formed
exactly in fp64 and rounded once to fp32 before the strict test: the kernel's single fma.

The bounds, from operation counts (not tuned):
  normals:  IrradianceGradReference.normal_bound with M and the slack taken with V, plus one
            2^-24 M for fp32(a v), plus 2^-25 per partly covered cell (0 < v < 1: v is one fp32
            fma, at most half an ulp of a number below 1 off) against its magnitude without v.
  weights:  IrradianceGradReference.weight_bound with M_k taken with V, plus the same two terms
            (fp32(cos v), and v's 2^-25 against the partly covered cells' magnitude without v).
  horizon:  1e-5 M + (sector_len + P + 6) 2^-24 M with M = n_z sum |d_out| |A| max(0, dot) over
            the row that counts (table rounding; the row's sum, the plane fold, and 6 for the dot
            product, to_local, the product with n_z and the two roundings of a term), plus
            "dot": 8 2^-24 n_z sum |d_out| |A| over that row without the cosine -- the rounding
            of the dot product and of to_local is absolute in the cosine, exactly the forward
            bound's 8 2^-24 A' (IrradianceReference.bound); without it a receiver that sees the
            row at grazing incidence has no allowance at all."""
import numpy as np

from sequence_irradiance_grad_reference import EPS, IrradianceGradReference
from sequence_irradiance_horizon_reference import HorizonReference


def frame_tables(seq):
    """(K, P, cells) fp64: every frame's own sky table, irradiance_frame_table(k)."""
    return np.stack([seq.irradiance_frame_table(k).astype(np.float64).reshape(seq.irradiance_info()["n_planes"], -1)
                     for k in range(len(seq))])


class HorizonGradReference:
    def __init__(self, seq, to_world=None):
        self.hz = HorizonReference(seq)
        self.g = IrradianceGradReference(seq, frame_tables(seq), to_world)
        self.r = self.g.r
        self.cells = self.r.n_z * self.r.n_phi

    # ------------------------------------------------------------ visibility
    def visibility(self, hp):
        """For (H, c) fp32 profiles: V (c, cells + K) fp64 -- v over the cells, 0 / 1 over the suns --
        and the mask (c, cells + K) of the partly covered cells (0 < v < 1)."""
        r = self.r
        sectors = hp.shape[0]
        length = r.n_phi // sectors
        top = np.arange(1, r.n_z + 1, dtype=np.float64)
        hh = hp.astype(np.float64).T                                                    # (c, H)
        v = np.clip(top[None, :, None] - hh[:, None, :] * r.n_z, 0.0, 1.0)            # (c, n_z, H)
        v = np.repeat(v, length, axis=2).reshape(hh.shape[0], -1)                       # (c, cells)
        visible = self.hz.sun_z32[None, :] >= hp[self.hz.cols // length, :].T           # (c, K), fp32 >= fp32
        V = np.concatenate([v, visible.astype(np.float64)], axis=1)
        part = np.concatenate([(v > 0) & (v < 1), np.zeros(visible.shape, bool)], axis=1)
        return V, part

    # ------------------------------------------------------------ normals
    def normal_grad(self, normals_local, d_out, h, chunk=256):
        """(grad, M, slack, partial), each (3, n), world space: IrradianceGradReference.normal_grad
        with V; partial = the magnitude without v of the partly covered cells in front."""
        g_ = self.g
        nl, d = np.asarray(normals_local, np.float64), np.asarray(d_out, np.float64)
        n = nl.shape[0]
        hp = self.hz.profiles(h, n)
        g, M, slack, partial = (np.zeros((3, n)) for _ in range(4))
        absdirs, absterms = np.abs(g_.dirs), np.abs(g_.terms)
        for lo in range(0, n, chunk):
            sl = slice(lo, lo + chunk)
            V, part = self.visibility(hp[:, sl])
            dots = nl[sl] @ g_.dirs.T
            a = d[:, sl].T @ g_.terms
            amag = np.abs(d[:, sl]).T @ absterms
            step = dots > 0
            near = np.abs(dots) < 8 * EPS * np.linalg.norm(nl[sl], axis=1, keepdims=True)
            g[:, sl] = ((a * V * step) @ g_.dirs).T
            M[:, sl] = ((amag * V * step) @ absdirs).T
            slack[:, sl] = ((np.abs(a) * V * near) @ absdirs).T
            partial[:, sl] = ((amag * (part & step)) @ absdirs).T
        aR = np.abs(g_.R)
        return g_.R @ g, aR @ M, aR @ slack, aR @ partial

    def normal_bound(self, M, slack, partial):
        return self.g.normal_bound(M, slack) + EPS * M + 0.5 * EPS * partial

    # ------------------------------------------------------------ weights
    def adjoint(self, normals_local, d_out, h, chunk=256):
        """(G, |G|, |G| of the partly covered cells without v), each (P, cells + K)."""
        g_ = self.g
        nl, d = np.asarray(normals_local, np.float64), np.asarray(d_out, np.float64)
        hp = self.hz.profiles(h, nl.shape[0])
        G, Gm, Gp = (np.zeros(g_.terms.shape) for _ in range(3))
        for lo in range(0, nl.shape[0], chunk):
            sl = slice(lo, lo + chunk)
            V, part = self.visibility(hp[:, sl])
            cos = np.maximum(nl[sl] @ g_.dirs.T, 0.0)
            G += d[:, sl] @ (cos * V)
            Gm += np.abs(d[:, sl]) @ (cos * V)
            Gp += np.abs(d[:, sl]) @ (cos * part)
        return G, Gm, Gp

    def weight_grad(self, normals_local, d_out, h):
        """(grad (K,), M (K,), partial (K,)); a frame whose sun is below the horizon gets exactly 0."""
        r, q = self.r, self.cells
        G, Gm, Gp = self.adjoint(normals_local, d_out, h)
        S = self.g.S
        gw = r.omega * np.einsum("pe,kpe->k", G[:, :q], S) + np.einsum("pk,pk->k", G[:, q:], r.F)
        M = r.omega * np.einsum("pe,kpe->k", Gm[:, :q], np.abs(S)) + np.einsum("pk,pk->k", Gm[:, q:], np.abs(r.F))
        partial = r.omega * np.einsum("pe,kpe->k", Gp[:, :q], np.abs(S))
        gw[r.suns[:, 2] < 0] = 0.0
        return gw, M, partial

    def weight_bound(self, M, partial, n, *cap):
        return self.g.weight_bound(M, n, *cap) + EPS * M + 0.5 * EPS * partial

    # ------------------------------------------------------------ the profile
    def horizon_grad(self, normals_local, d_out, h, chunk=256):
        """(grad, M, flat), each (H, n): one value per (sector, receiver), also for a shared profile.
        M = n_z sum |d_out| |A| max(0, dot) over the partly covered row, flat the same without the
        cosine."""
        r, g_ = self.r, self.g
        nl, d = np.asarray(normals_local, np.float64), np.asarray(d_out, np.float64)
        n = nl.shape[0]
        hp = self.hz.profiles(h, n)
        sectors = hp.shape[0]
        length = r.n_phi // sectors
        top = np.arange(1, r.n_z + 1, dtype=np.float64)
        sky, abssky = g_.terms[:, :self.cells], np.abs(g_.terms[:, :self.cells])
        out, M, flat = (np.zeros((sectors, n)) for _ in range(3))
        for lo in range(0, n, chunk):
            sl = slice(lo, lo + chunk)
            hh = hp[:, sl].astype(np.float64).T                                          # (c, H)
            t = (top[None, :, None] - hh[:, None, :] * r.n_z).astype(np.float32)        # exact, rounded once
            cut = (t > 0) & (t < 1)                                                      # (c, n_z, H)
            assert cut.sum(1).max() <= 1                                                 # at most one row per sector
            cos = np.maximum(nl[sl] @ r.centres.T, 0.0)
            a = d[:, sl].T @ sky
            amag = np.abs(d[:, sl]).T @ abssky
            shape = (-1, r.n_z, sectors, length)
            out[:, sl] = (-r.n_z * ((cos * a).reshape(shape).sum(3) * cut).sum(1)).T
            M[:, sl] = (r.n_z * ((cos * amag).reshape(shape).sum(3) * cut).sum(1)).T
            flat[:, sl] = (r.n_z * (amag.reshape(shape).sum(3) * cut).sum(1)).T
        return out, M, flat

    def horizon_bound(self, M, flat, sectors):
        r = self.r
        return 1e-5 * M + (r.n_phi // sectors + r.planes + 6) * EPS * M + 8 * EPS * flat
