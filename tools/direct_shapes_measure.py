"""Figures behind tests/test_gpu_direct_shapes.py::test_seeds_at_the_ends_of_the_range and DESIGN.md
section 6 (measured only, nothing asserted):
  1. the seed test's statistics (rays-parity bounds) at 1024 points, spp 3 and 48, with the parity
     tests' normals and views (input seed 8) and with another set (input seed 67);
  2. where the BSDF rays over 5e-4 sit: per input set, seed and spp the rays over 5e-4, the points
     they belong to and those points' cos_i (views within 2 degrees of the normal).
usage: python tools/direct_shapes_measure.py > profiles/direct_shapes_measure.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("oracle", "mitsuba3-sunsky_amd", "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import oracle as O  # noqa: E402
import gpu_direct_worker as W  # noqa: E402
import test_direct_shapes_cpu as R  # noqa: E402

torch.cuda.set_device(0)
print("== 1. the seed test's statistics at 1024 points")
for precision in ("fast", "reference"):
    em = W.emitter("rgb", precision)
    o32 = R.make_oracle("identity", "base", "rgb", w_sky=em.sky_sampling_w)
    for inseed in (8, 67):
        for spp in (3, 48):
            inp = W.inputs(1024, spp, seed=inseed)
            t = W.to_gpu(inp)
            for seed in (0, 0xFFFFFFFF):
                got = {k: v for k, v in W.run_direct(em, t, seed, spp, conductors=R.DEG_CONDUCTORS).items()
                       if "raysw" in k or k.startswith("diffuse_rays")}
                ref = {k: v for k, v in R.reference(o32, inp, seed, spp, conductors=R.DEG_CONDUCTORS).items() if "rays" in k}
                g = {k: (R.rays_np(v) if k.endswith(("_em", "_bs")) else v.cpu().numpy()) for k, v in got.items()}
                for k in ref:
                    if k.endswith(("_bs", "_bw")) and k.startswith("conductor"):
                        try:
                            R.check_all(g, {k: ref[k]}, f"{precision} inputs {inseed} spp {spp} seed {seed:#x}")
                        except AssertionError:
                            print(f"   ^ outside the rays-parity bound: {k}")
print("== 2. BSDF rays over 5e-4 by view")
for precision in ("fast", "reference"):
    em = W.emitter("rgb", precision)
    o32 = R.make_oracle("identity", "base", "rgb", w_sky=em.sky_sampling_w)
    for n, inseed in ((1024, 8), (1024, 67), (1024, 68), (1024, 69), (1024, 70), (16384, 67)):
        inp = W.inputs(n, 16, seed=inseed)
        t = W.to_gpu(inp)
        cosv = (inp["nrm"] * inp["wi"]).sum(0)
        for dist, alpha in (("beckmann", 0.25), ("ggx", (0.08, 0.35))):
            for seed in (0, 0xFFFFFFFF, 21):
                for spp in (3, 16):
                    e, b = em.direct_conductor_rays(t["nrm"], t["wi"], alpha, dist, seed, spp)
                    g = R.rays_np(b)
                    eo, bo = O.direct_conductor_rays(o32, inp["nrm"].T, inp["wi"].T, alpha, dist, seed, spp)
                    both = g.any(2) & bo.any(2)
                    d = np.where(both, np.abs(g.astype(np.float64) - bo).max(2), 0)
                    bad = d > 5e-4
                    pts = np.unique(np.nonzero(bad)[1])
                    print(f"{precision} n={n} inputs {inseed} {dist} {alpha} seed={seed:#x} spp={spp}: rays {both.sum()} "
                          f"p99.9 {np.quantile(d[both], 0.999):.2e} max {d.max():.2e} over 5e-4: {bad.sum()} "
                          f"({bad.sum() / both.sum():.2e}) on {len(pts)} points, cos_i {np.round(cosv[pts][:8], 4)}", flush=True)
