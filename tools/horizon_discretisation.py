"""Discretisation of the occluded sky part of sequence.irradiance(horizon=...), on the CPU.

The five-frame test sky (tests/sequence_cases.py), RGB, host-only tables.  Per profile, table and
receiver normal: the sky part of E by the header's rule (the visible share v of a cut cell,
fractional) and by the centre-only binary rule (v = 1 where the cell centre lies above the
horizon, else 0), each against a converged quadrature of the fp64 oracle's sky that integrates
the same sector-wise horizon exactly: per sector Gauss-Legendre in z from h to 1 (768 nodes) times
the midpoint rule in azimuth (1536 columns over the circle; the sector edges are column edges).
Prints the worst relative error over the six normals and the three planes.  No gate: the figures
are recorded in DESIGN.md.

usage: python tools/horizon_discretisation.py"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in ("mitsuba3-sunsky_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import oracle as O  # noqa: E402
import sunsky_amd as ss  # noqa: E402
from sequence_cases import TURBIDITY, WEIGHTS, base_dict, frame_dict, frame_dirs  # noqa: E402
from sequence_sampling_reference import cell_centres  # noqa: E402

N_MU, N_PHI = 768, 1536
T35, D30 = np.deg2rad(35.0), np.deg2rad(30.0)
NORMALS = {"horizontal": [0, 0, 1], "35 degree tilt": [np.sin(T35) * np.cos(0.3), np.sin(T35) * np.sin(0.3), np.cos(T35)],
           "vertical +x": [1, 0, 0], "vertical +y": [0, 1, 0], "vertical -x-y": [-np.sqrt(0.5), -np.sqrt(0.5), 0],
           "30 degrees down": [np.cos(D30) * np.cos(2.0), np.cos(D30) * np.sin(2.0), -np.sin(D30)]}


def profile(name, sectors):
    """sin(horizon elevation) per sector, fp32 as the kernel takes it."""
    deg = np.full(sectors, 10.0)
    if name == "10 degrees + a 40 degree wall over [0, 90) degrees":
        deg[:sectors // 4] = 40.0
    return ss.horizon_from_elevation(deg)


PROFILES = ["10 degrees everywhere", "10 degrees + a 40 degree wall over [0, 90) degrees"]


def exact_radiance(h):
    """The weighted fp64 sky on the N_MU x N_PHI grid over z in [h, 1]: (3, N_MU, N_PHI), the
    directions (N_MU, N_PHI, 3) and the Gauss-Legendre weights."""
    x, w = np.polynomial.legendre.leggauss(N_MU)
    mu, wmu = 0.5 * (1 - h) * x + 0.5 * (1 + h), 0.5 * (1 - h) * w
    phi = (np.arange(N_PHI) + 0.5) * (2 * np.pi / N_PHI)
    st = np.sqrt(1 - mu * mu)
    d = np.stack([np.outer(st, np.cos(phi)), np.outer(st, np.sin(phi)), np.repeat(mu[:, None], N_PHI, 1)], -1)
    L = np.zeros((3, N_MU * N_PHI))
    dirs = frame_dirs()
    for k, wk in enumerate(WEIGHTS):
        if wk == 0 or dirs[k][2] < 0:
            continue
        o = O.Oracle(dict(frame_dict(base_dict(), dirs[k], TURBIDITY[k]), sun_scale=0.0), "rgb", "jit", "f64")
        L += wk * np.asarray(o.eval(-d.reshape(-1, 3).astype(np.float32)), np.float64).T
    return L.reshape(3, N_MU, N_PHI), d, wmu


def main():
    parent = ss.SunskyEmitter(base_dict(), variant="rgb", device="host")
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    normals = np.asarray(list(NORMALS.values()), np.float64)
    grids = {}
    for name in PROFILES:
        for (nz, nphi), sectors in (((16, 32), 8), ((64, 256), 32)):
            h = profile(name, sectors).astype(np.float64)
            # the converged value, sector by sector
            exact = np.zeros((3, len(normals)))
            per = N_PHI // sectors
            for b in range(sectors):
                if h[b] not in grids:
                    grids[h[b]] = exact_radiance(h[b])
                L, d, wmu = grids[h[b]]
                cols = slice(b * per, (b + 1) * per)
                cos = np.maximum(d[:, cols] @ normals.T, 0.0)                                # (N_MU, per, normals)
                exact += np.einsum("pmj,mjn,m->pn", L[:, :, cols], cos, wmu) * (2 * np.pi / N_PHI)
            # the table's two rules
            seq.prepare_irradiance(nz, nphi)
            terms = float(seq.irradiance_info()["omega"]) * seq.irradiance_table("sky").astype(np.float64).reshape(3, -1)
            cos = np.maximum(cell_centres(nz, nphi) @ normals.T, 0.0)                        # (cells, normals)
            hb = np.repeat(h, nphi // sectors)                                               # per column
            top = np.arange(1, nz + 1)[:, None]
            share = np.clip(top - hb[None, :] * nz, 0.0, 1.0).reshape(-1)
            centre = (((np.arange(nz) + 0.5) / nz)[:, None] >= hb[None, :]).astype(np.float64).reshape(-1)
            line = [f"{name}: {nz} x {nphi}, H = {sectors}:"]
            for rule, v in (("fractional", share), ("centre-only binary", centre)):
                e = terms @ (cos * v[:, None])
                rel = np.abs(e - exact) / np.abs(exact)
                line.append(f"{rule} worst {rel.max():.2e} ({list(NORMALS)[int(rel.max(0).argmax())]})")
            print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
