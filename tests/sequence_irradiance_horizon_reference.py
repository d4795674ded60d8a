"""numpy restatement of a sequence's irradiance under a horizon profile (include/sunsky_amd.h,
"the irradiance under a horizon profile") over the tables read back from the product:

    v_r[i, b] = min(max(i + 1 - h_r[b] n_z, 0), 1)
    E_p(n_r; h_r) = sum_ij omega R_p[i, j] max(0, n_l . c_ij) v_r[i, b(j)]
                  + sum_k [s_k.z >= h_r[b_k]] w_k F_k[p] max(0, n_l . s_k)

in fp64: v in fp64 from the fp32 h (the product h n_z is exact in fp64, so v is the exact visible
share), the sun's visibility by the exact fp32 comparison, its sector from
irradiance_sun_columns().

The rounding bound.  It starts from IrradianceReference.bound,
    1e-5 A + 8 2^-24 A' + (n_phi + n_z + K + 4) 2^-24 A
(table rounding; rounding of the dot product and of to_local against the terms without the
cosine, A'; accumulation depth), with A = sum |terms| taken with the cosine AND the visibility,
since v <= 1 multiplies the cosine before anything is added and a hidden sun adds nothing.  The
kernel does two things more than the forward, counted from the operations, not tuned:
  - per term one more rounding, fp32(c v): 2^-24 relative to the term, so one more 2^-24 A;
  - v itself is one fp32 fma, rounded once: v lies in [0, 1], so where it is not exactly 0 or 1
    its error is at most half an ulp of a number below 1, 2^-25 absolute; a row has such cells in
    the sectors its horizon cuts only, at most n_phi cells per receiver (one row per sector).
    Absolute in v means relative to the term without v: 2^-25 times the sum over the partly
    covered cells of |omega R| max(0, n_l . c), `partial` below, which is at most A'.
Where v is exactly 0 or 1 in fp64 the fp32 fma gives the same 0 or 1 (the clamp of a correctly
rounded value), so those cells carry no v error."""
import numpy as np

from sequence_irradiance_reference import IrradianceReference


class HorizonReference(IrradianceReference):
    def __init__(self, seq):
        super().__init__(seq)
        self.cols = np.asarray(seq.irradiance_sun_columns(), np.int64)
        assert self.cols.shape == (self.K,)
        self.sun_z32 = self.suns[:, 2].astype(np.float32)   # the frames' fp32 values, exactly

    def profiles(self, h, n):
        """(H, n) fp32 profiles from (H,), (H, 1) or (H, n)."""
        h = np.asarray(h, np.float32)
        h = h[:, None] if h.ndim == 1 else h
        assert self.n_phi % h.shape[0] == 0 and h.shape[1] in (1, n)
        return np.broadcast_to(h, (h.shape[0], n))

    def parts(self, normals_local, h, chunk=512):
        """(E_sky, E_sun, A, partial), each (P, n), for (n, 3) local normals under the profiles h:
        A = sum |terms| with the cosine and the visibility, partial = the same sum without v over
        the cells a horizon cuts (0 < v < 1)."""
        nl = np.asarray(normals_local, np.float64)
        n = nl.shape[0]
        hp = self.profiles(h, n)
        sectors = hp.shape[0]
        length = self.n_phi // sectors
        top = np.arange(1, self.n_z + 1, dtype=np.float64)
        sky, mag, partial = (np.empty((self.planes, n)) for _ in range(3))
        for a in range(0, n, chunk):
            hh = hp[:, a:a + chunk].astype(np.float64).T                                  # (c, H)
            v = np.clip(top[None, :, None] - hh[:, None, :] * self.n_z, 0.0, 1.0)       # (c, n_z, H)
            v = np.repeat(v, length, axis=2).reshape(hh.shape[0], -1)                     # (c, cells)
            cos = np.maximum(nl[a:a + chunk] @ self.centres.T, 0.0)
            cv = cos * v
            sky[:, a:a + chunk] = self.sky_terms @ cv.T
            mag[:, a:a + chunk] = np.abs(self.sky_terms) @ cv.T
            partial[:, a:a + chunk] = np.abs(self.sky_terms) @ (cos * ((v > 0) & (v < 1))).T
        visible = self.sun_z32[None, :] >= hp[self.cols // length, :].T                   # (n, K), fp32 >= fp32
        cos = np.maximum(nl @ self.suns.T, 0.0) * visible
        return sky, self.sun_terms @ cos.T, mag + np.abs(self.sun_terms) @ cos.T, partial

    def bound(self, A, partial):
        eps = 2.0 ** -24
        return IrradianceReference.bound(self, A) + eps * A + 0.5 * eps * partial
