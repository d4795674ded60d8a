"""numpy restatement of a sequence's sampling distribution (include/sunsky_amd.h, "importance
sampling of a sequence"): the pdf and the sample map over the tables read back from the product,
the way the kernel-isolating sampler tests adopt the product's state.  All in the local frame.

    pdf(d) = w_sky f_cell(d) / (S omega) + (1 - w_sky) sun_pdf sum_k q_k [dot(s_k, d) >= cos_cutoff]

The CDF inversions run in fp32 with the kernel's operations (so the picked entry and the reused
sample are the kernel's wherever u is not within rounding of a CDF entry); the geometry after
them runs in fp64.  Every function also returns the lanes whose result hangs on an fp32 rounding
(a cell boundary, a cone edge, a CDF entry), which the tests leave out under a cap.
"""
import numpy as np

CIE_Y_NODES = np.array([0.0, 3.917e-06, 0.000396, 0.023, 0.13902, 0.71, 0.995, 0.631, 0.175, 0.017, 0.001047])
NODE_LAMBDAS = [320.0 + 40.0 * c for c in range(11)]
LUM_RGB = np.array([0.212671, 0.715160, 0.072169])
ONE_MINUS_EPS = np.float32(0.99999994039535522461)
F32 = np.float32


def luminance(v, spectral):
    """Y of (..., C) values: the RGB luminance weights or sum_c cie_y[c] L_c / 11 over the 11 nodes."""
    v = np.asarray(v, np.float64)
    return v @ CIE_Y_NODES / 11.0 if spectral else v @ LUM_RGB


def cell_centres(n_z, n_phi):
    """(n_z * n_phi, 3) local directions of the cell centres, row-major, fp64."""
    z = (np.arange(n_z) + 0.5) / n_z
    phi = (np.arange(n_phi) + 0.5) * (2 * np.pi / n_phi)
    st = np.sqrt(1 - z * z)
    return np.stack([np.outer(st, np.cos(phi)).ravel(), np.outer(st, np.sin(phi)).ravel(),
                     np.repeat(z, n_phi)], 1)


def _coordinate_system(n):
    """coordinate_system (vector.h:116-137) of one fp64 vector."""
    sign = np.copysign(1.0, n[2])
    a = -1.0 / (sign + n[2])
    b = n[0] * n[1] * a
    return (np.array([sign * n[0] * n[0] * a + 1.0, sign * b, -sign * n[0]]),
            np.array([b, n[1] * n[1] * a + sign, -n[1]]))


def _uniform_cone(sx, sy, cos_cutoff):
    """square_to_uniform_cone over the concentric disk (warp.h:54-90, 533-551), fp64."""
    x, y = 2 * sx - 1, 2 * sy - 1
    q13 = np.abs(x) < np.abs(y)
    r, rp = np.where(q13, y, x), np.where(q13, x, y)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = 0.25 * np.pi * rp / r
    phi = np.where(q13, 0.5 * np.pi - phi, phi)
    phi = np.where((x == 0) & (y == 0), 0.0, phi)
    px, py = r * np.cos(phi), r * np.sin(phi)
    omc = 1.0 - cos_cutoff
    pn = px * px + py * py
    sc = np.sqrt(np.maximum(omc * (2 - omc * pn), 0))
    return px * sc, py * sc, cos_cutoff + omc * (1 - pn)


class SamplingReference:
    def __init__(self, seq, cos_cutoff):
        i = seq.sampling_info()
        self.n_z, self.n_phi, self.w_sky = i["n_z"], i["n_phi"], F32(i["w_sky"])
        self.f = seq.sampling_table("sky")
        self.row_cdf, self.cell_cdf = seq.sampling_table("row_cdf"), seq.sampling_table("cell_cdf")
        self.q, self.frame_cdf, self.B = (seq.sampling_table(n) for n in ("q", "frame_cdf", "B"))
        self.K = len(self.q)
        self.suns = np.stack([seq.frame(k)["sun_dir_local"] for k in range(self.K)]).astype(np.float32)
        self.weights = np.array([seq.frame(k)["weight"] for k in range(self.K)], np.float64)
        self.cos_cutoff = F32(cos_cutoff)
        self.sun_pdf = F32(0.15915494309189533577) / (F32(1) - self.cos_cutoff)   # warp.h:568-577
        self.S = float(self.f.astype(np.float64).sum())
        self.omega = 2 * np.pi / (self.n_z * self.n_phi)
        self.dphi = 2 * np.pi / self.n_phi

    # ---------------------------------------------------------------- derived scalars
    def masses(self):
        """(M, P, w_sky) recomputed from the read-backs in fp64."""
        M = self.S * self.omega
        P = 2 * np.pi * (1.0 - float(self.cos_cutoff)) * float(self.weights @ self.B.astype(np.float64))
        return M, P, M / (M + P)

    # ---------------------------------------------------------------- pdf
    def cone_hits(self, d):
        """(n, K) cone membership dot(s_k, d) >= cos_cutoff in fp64 over the fp32 inputs, and the
        lanes within 3e-7 of an edge (only cones that carry probability count)."""
        dots = np.asarray(d, np.float64) @ self.suns.astype(np.float64).T
        edge = (np.abs(dots - float(self.cos_cutoff)) < 3e-7) & (self.q > 0)[None, :]
        return dots >= float(self.cos_cutoff), edge.any(axis=1)

    def cells(self, d):
        """Cell (row, column) of local directions and the lanes within 2^-20 of a row boundary in z
        or 1e-5 rad of a column boundary."""
        d = np.asarray(d, np.float64)
        zr = d[:, 2] * self.n_z
        row = np.clip(np.floor(zr), 0, self.n_z - 1).astype(int)
        phi = np.mod(np.arctan2(d[:, 1], d[:, 0]), 2 * np.pi)
        pc = phi / self.dphi
        col = np.clip(np.floor(pc), 0, self.n_phi - 1).astype(int)
        # z = 1 belongs to the last row: the top of the table is no boundary
        near_row = (np.abs(zr - np.round(zr)) < 2.0 ** -20 * self.n_z) & (np.round(zr) < self.n_z)
        near_col = np.abs(pc - np.round(pc)) * self.dphi < 1e-5
        return row, col, near_row | near_col

    def pdf(self, d, active=None, resolve=None):
        """(pdf fp64, leave_out) at local directions d (n, 3).  Left out: lanes at a cell boundary
        and lanes within 3e-7 of a cone edge, where the fp32 dot decides.  With `resolve` (the
        kernel's pdf of the same lanes) a lane at ONE cone's edge is not left out: it has two
        admissible values, that cone counted or not, and the nearer to `resolve` is returned --
        the caller's bar then holds the kernel to one of the two.  (A sampled sun pick lies in
        that band with probability 3e-7 / (1 - cos_cutoff), 2.7 % at the default aperture.)"""
        d = np.asarray(d, np.float64)
        row, col, near = self.cells(d)
        dots = d @ self.suns.astype(np.float64).T
        cc, q = float(self.cos_cutoff), self.q.astype(np.float64)
        amb = (np.abs(dots - cc) < 3e-7) & (q > 0)[None, :]
        sure = (dots >= cc) & ~amb
        coef = (1.0 - float(self.w_sky)) * float(self.sun_pdf)
        sky = float(self.w_sky) * self.f[row, col].astype(np.float64) / (self.S * self.omega) if self.S > 0 else 0.0
        lo = sky + coef * (sure * q[None, :]).sum(1)
        hi = lo + coef * (amb * q[None, :]).sum(1)
        if resolve is None:
            p, edge = sky + coef * ((dots >= cc) * q[None, :]).sum(1), amb.any(axis=1)
        else:
            r = np.asarray(resolve, np.float64)
            p, edge = np.where(np.abs(r - hi) < np.abs(r - lo), hi, lo), amb.sum(axis=1) > 1
        p = np.where(d[:, 2] >= 0, p, 0.0)
        if active is not None:
            p = np.where(np.asarray(active, bool), p, 0.0)
        return p, (near | edge) & (d[:, 2] >= 0)

    # ---------------------------------------------------------------- sample map
    @staticmethod
    def _invert(cdf_rows, u):
        """Per lane: first entry of its (inclusive, normalised) CDF above u, the reused sample in
        [0, 1) and the distance of u to the nearest entry -- fp32, the kernel's operations."""
        n = cdf_rows.shape[-1]
        if cdf_rows.ndim == 1:
            j = np.minimum(np.searchsorted(cdf_rows, u, side="right"), n - 1)
            lo = np.where(j > 0, cdf_rows[np.maximum(j - 1, 0)], F32(0))
            hi = cdf_rows[j]
            gap = np.abs(cdf_rows[None, :].astype(np.float64) - u[:, None]).min(1)
        else:
            j = np.minimum((cdf_rows <= u[:, None]).sum(1), n - 1)
            r = np.arange(len(u))
            lo = np.where(j > 0, cdf_rows[r, np.maximum(j - 1, 0)], F32(0))
            hi = cdf_rows[r, j]
            gap = np.abs(cdf_rows.astype(np.float64) - u[:, None]).min(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(hi > lo, (u - lo) / (hi - lo), F32(0)).astype(np.float32)
        return j, np.clip(t, F32(0), ONE_MINUS_EPS), gap

    def sample(self, u):
        """u (2, n) fp32 -> dict: d (n, 3) local fp64, pick_sky, the picked (row, col) / frame,
        the in-cell position (t1, t2), active (z >= 0), leave_out (u1, u1' or u2 within 1e-6 of a
        CDF entry or of w_sky)."""
        u1, u2 = (np.asarray(x, np.float32) for x in u)
        n = u1.shape[0]
        w = self.w_sky
        sky = u1 < w
        d = np.zeros((n, 3))
        out = {"pick_sky": sky, "row": np.full(n, -1), "col": np.full(n, -1), "frame": np.full(n, -1),
               "t1": np.zeros(n, np.float32), "t2": np.zeros(n, np.float32)}
        leave = np.abs(u1.astype(np.float64) - float(w)) < 1e-6
        if sky.any():
            a = np.minimum(u1[sky] / w, ONE_MINUS_EPS)
            i, t2, g2 = self._invert(self.row_cdf, u2[sky])
            j, t1, g1 = self._invert(self.cell_cdf[i], a)
            z = np.minimum((i.astype(np.float32) + t2) / F32(self.n_z), F32(1)).astype(np.float64)
            phi = ((j.astype(np.float32) + t1) * F32(self.dphi)).astype(np.float64)
            st = np.sqrt(np.maximum(1 - z * z, 0))
            d[sky] = np.stack([st * np.cos(phi), st * np.sin(phi), z], 1)
            out["row"][sky], out["col"][sky], out["t1"][sky], out["t2"][sky] = i, j, t1, t2
            leave[sky] |= (g1 < 1e-6) | (g2 < 1e-6)
        sun = ~sky
        if sun.any():
            with np.errstate(invalid="ignore", divide="ignore"):
                a = np.minimum((u1[sun] - w) / (F32(1) - w), ONE_MINUS_EPS).astype(np.float32)
            k, t1, g = self._invert(self.frame_cdf, a)
            x, y, zc = _uniform_cone(t1.astype(np.float64), u2[sun].astype(np.float64), float(self.cos_cutoff))
            ds = np.zeros((k.shape[0], 3))
            for kk in np.unique(k):
                s = self.suns[kk].astype(np.float64)
                fs, ft = _coordinate_system(s)
                m = k == kk
                ds[m] = x[m, None] * fs + y[m, None] * ft + zc[m, None] * s
            ds[:, 2] = np.minimum(ds[:, 2], 1.0)   # cos theta <= 1, as the sky pick's min()
            d[sun] = ds
            out["frame"][sun], out["t1"][sun] = k, t1
            leave[sun] |= g < 1e-6
        out.update(d=d, active=d[:, 2] >= 0, leave_out=leave)
        return out
