"""numpy restatement of a sequence's per-frame irradiance series (include/sunsky_amd.h, "the
per-frame irradiance series") over the tables read back from the product:

    E^k_p(n)      = sum_ij omega sky_{k,p}(c_ij) max(0, n_l . c_ij) + F_k[p] max(0, n_l . s_k)
    E^k_p(n; h_r) = sum_ij omega sky_{k,p}(c_ij) max(0, n_l . c_ij) v_r[i, b(j)]
                  + [s_k.z >= h_r[b_k]] F_k[p] max(0, n_l . s_k)

in fp64: sky_{k,p} from irradiance_frame_table(k), F from the "sun_flux" table, s_k from frame(k),
the sun's sector from irradiance_sun_columns(), v and the sun's visibility as
tests/sequence_irradiance_horizon_reference.py forms them.  The weights do not enter.

The rounding bound is IrradianceReference.bound / HorizonReference.bound with K replaced by 1,
since every frame and plane is the irradiance of a sequence that holds that frame alone:
    1e-5 A + 8 2^-24 A' + (n_phi + n_z + 1 + 4) 2^-24 A     [+ 2^-24 A + 2^-25 partial under a horizon]
with, per frame and plane, A = sum |terms| with the cosine (and the visibility), A' the same sum
without the cosine and `partial` the sum without v over the cells a horizon cuts; their derivation
is in the two modules named."""
import numpy as np

from sequence_sampling_reference import cell_centres


class SeriesReference:
    def __init__(self, seq):
        i = seq.irradiance_info()
        self.n_z, self.n_phi, self.planes = i["n_z"], i["n_phi"], i["n_planes"]
        self.K = len(seq)
        self.omega = float(i["omega"])
        self.tables = np.stack([seq.irradiance_frame_table(k) for k in range(self.K)])     # (K, P, n_z, n_phi) fp32
        self.F = seq.irradiance_table("sun_flux").astype(np.float64).T.copy()              # (K, P)
        frames = [seq.frame(k) for k in range(self.K)]
        self.suns = np.array([f["sun_dir_local"] for f in frames], np.float64)
        self.w = np.array([f["weight"] for f in frames], np.float64)
        self.sun_z32 = self.suns[:, 2].astype(np.float32)
        self.cols = np.asarray(seq.irradiance_sun_columns(), np.int64)
        self.centres = cell_centres(self.n_z, self.n_phi)
        self.sky_terms = self.omega * self.tables.astype(np.float64).reshape(self.K * self.planes, -1)
        # A': the terms without the cosine, per frame and plane
        self.flat = np.abs(self.sky_terms).sum(1).reshape(self.K, self.planes) + np.abs(self.F)

    def parts(self, normals_local, h=None, chunk=512):
        """(E_sky, E_sun, A, partial), each (K, P, n), for (n, 3) local normals, under the profiles h
        ((H,), (H, 1) or (H, n) fp32) when given; partial is 0 without a horizon."""
        nl = np.asarray(normals_local, np.float64)
        n, KP = nl.shape[0], self.K * self.planes
        sky, mag, partial = (np.zeros((KP, n)) for _ in range(3))
        if h is not None:
            hp = np.asarray(h, np.float32)
            hp = hp[:, None] if hp.ndim == 1 else hp
            assert self.n_phi % hp.shape[0] == 0 and hp.shape[1] in (1, n)
            hp = np.broadcast_to(hp, (hp.shape[0], n))
            length = self.n_phi // hp.shape[0]
            top = np.arange(1, self.n_z + 1, dtype=np.float64)
        absterms = np.abs(self.sky_terms)
        for a in range(0, n, chunk):
            cos = np.maximum(nl[a:a + chunk] @ self.centres.T, 0.0)
            cv = cos
            if h is not None:
                hh = hp[:, a:a + chunk].astype(np.float64).T                                  # (c, H)
                v = np.clip(top[None, :, None] - hh[:, None, :] * self.n_z, 0.0, 1.0)       # (c, n_z, H)
                v = np.repeat(v, length, axis=2).reshape(hh.shape[0], -1)                     # (c, cells)
                cv = cos * v
                partial[:, a:a + chunk] = absterms @ (cos * ((v > 0) & (v < 1))).T
            sky[:, a:a + chunk] = self.sky_terms @ cv.T
            mag[:, a:a + chunk] = absterms @ cv.T
        cos = np.maximum(nl @ self.suns.T, 0.0)                                               # (n, K)
        if h is not None:
            cos = cos * (self.sun_z32[None, :] >= hp[self.cols // length, :].T)               # fp32 >= fp32
        sun = self.F[:, :, None] * cos.T[:, None, :]                                          # (K, P, n)
        shape = (self.K, self.planes, n)
        return sky.reshape(shape), sun, mag.reshape(shape) + np.abs(sun), partial.reshape(shape)

    def bound(self, A, partial=None):
        """Per frame, plane and receiver; partial: under a horizon."""
        eps = 2.0 ** -24
        b = 1e-5 * A + 8 * eps * self.flat[:, :, None] + (self.n_phi + self.n_z + 1 + 4) * eps * A
        return b if partial is None else b + eps * A + 0.5 * eps * partial
