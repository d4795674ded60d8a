"""numpy restatement of a sequence's irradiance (include/sunsky_amd.h, "irradiance of the
cumulative sky on oriented receivers") over the tables read back from the product:

    E_p(n) = sum_ij omega R_p[i, j] max(0, n_l . c_ij) + sum_k w_k F_k[p] max(0, n_l . s_k)

in fp64, with the magnitudes the rounding bound of tests/test_gpu_sequence_irradiance.py needs."""
import numpy as np

from sequence_sampling_reference import cell_centres


class IrradianceReference:
    def __init__(self, seq):
        i = seq.irradiance_info()
        self.n_z, self.n_phi, self.planes = i["n_z"], i["n_phi"], i["n_planes"]
        self.K = len(seq)
        self.omega = float(i["omega"])
        self.R = seq.irradiance_table("sky").astype(np.float64).reshape(self.planes, -1)
        self.F = seq.irradiance_table("sun_flux").astype(np.float64)
        frames = [seq.frame(k) for k in range(self.K)]
        self.suns = np.array([f["sun_dir_local"] for f in frames], np.float64)
        self.w = np.array([f["weight"] for f in frames], np.float64)
        self.centres = cell_centres(self.n_z, self.n_phi)
        self.sky_terms = self.omega * self.R          # (P, cells)
        self.sun_terms = self.w[None, :] * self.F     # (P, K)
        # A': the terms without the cosine
        self.flat = np.abs(self.sky_terms).sum(1) + np.abs(self.sun_terms).sum(1)

    def parts(self, normals_local, chunk=512):
        """(E_sky, E_sun, A), each (P, n), for (n, 3) local normals; A = sum |terms| with the cosine."""
        nl = np.asarray(normals_local, np.float64)
        sky, mag = np.empty((self.planes, nl.shape[0])), np.empty((self.planes, nl.shape[0]))
        for a in range(0, nl.shape[0], chunk):
            cos = np.maximum(nl[a:a + chunk] @ self.centres.T, 0.0)
            sky[:, a:a + chunk] = self.sky_terms @ cos.T
            mag[:, a:a + chunk] = np.abs(self.sky_terms) @ cos.T
        cos = np.maximum(nl @ self.suns.T, 0.0)
        return sky, self.sun_terms @ cos.T, mag + np.abs(self.sun_terms) @ cos.T

    def bound(self, A):
        """Per plane and receiver: table rounding, rounding of the dot product and of to_local,
        accumulation depth."""
        eps = 2.0 ** -24
        return 1e-5 * A + 8 * eps * self.flat[:, None] + (self.n_phi + self.n_z + self.K + 4) * eps * A
