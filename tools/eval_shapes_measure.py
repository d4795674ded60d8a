"""Figures behind tests/test_gpu_eval_shapes.py and DESIGN.md section 6 "Eval and bake call shapes"
(measured only, nothing asserted):
  1. per bake case (variant, precision, frame, wavelength list, image): the worst ratio of
     |bake - o64| to the bound of eval_shapes_reference.BakeReference for the GPU and for the fp32
     oracle, the loose pixels, and the pixels structurally below the horizon that are not 0;
  2. per eval case (entry point, wavelength count or list, precision, frame) at 4099 directions:
     helpers.parity_stats against the two oracles;
  3. per sequence bake case: the worst ratio to the weighted sum of the per-frame bounds.
usage: python tools/eval_shapes_measure.py > profiles/eval_shapes_measure.log"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("oracle", "mitsuba3-sunsky_amd", "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import eval_shapes_reference as R  # noqa: E402
import gpu_eval_worker as W  # noqa: E402
import sequence_cases as SC  # noqa: E402
import sunsky_amd as ss  # noqa: E402
from helpers import parity_stats  # noqa: E402

torch.cuda.set_device(0)
N = 4099
PRECISIONS = ("fast", "reference")

print("== 1. the bake against the oracle")
print("variant | frame | list | image | pixels | loose | o32 ratio | fast ratio | reference ratio | dark pixels lit")
for variant in ("rgb", "spectral"):
    for frame in R.FRAMES:
        ems = {p: W.emitter(variant, p, frame) for p in PRECISIONS}
        for lname, lam in R.bake_lists(variant).items():
            for image, w, h, theta, phi, cap in R.bake_images(frame):
                ref = R.BakeReference(variant, frame, w, h, theta, phi, lam)
                worst, lit = {}, 0
                for p, em in ems.items():
                    img = em.bake_latlong(w, h, theta, phi, wavelengths=lam).cpu().numpy().reshape(-1, w * h)
                    worst[p] = ref.ratio(img).max()
                    lit += int((img[:, ref.dark] != 0).any(axis=0).sum())
                print(f"{variant} | {frame} | {lname} | {image} | {w * h} | {int(ref.loose.sum())} | "
                      f"{ref.ratio(ref.o32).max():.3f} | {worst['fast']:.3f} | {worst['reference']:.3f} | {lit}", flush=True)

print("== 2. eval against the oracle, 4099 directions (parity_stats)")
for frame in R.FRAMES:
    inp = R.inputs(N, frame)
    sun = R.sun_lanes(frame, inp["wo"].T)
    for variant in ("rgb", "spectral"):
        o32, o64 = R.oracles(variant, frame)
        if variant == "rgb":
            cases = [("eval", "eval", None, 0), ("eval_direction", "eval_direction", None, 0)]
        else:
            cases = [(f"{e} nlam={k}", e, inp["lam"][:k], k) for e in ("eval", "eval_direction") for k in (2, 4, 9, 16)]
            cases += [(f"broadcast {name}", "broadcast", lam, 0) for name, lam in
                      (("m1", [555.0]), ("nodes", R.NODES), ("reversed", R.NODES[::-1]), ("m32", R.LIST32))]
        for name, entry, lam, nlam in cases:
            a, b = R.oracle_eval(o32, inp["wo"].T, lam), R.oracle_eval(o64, inp["wo"].T, lam)
            for p in PRECISIONS:
                got, lost = W.eval_call(W.emitter(variant, p, frame), entry, inp["wo"], inp["lam"] if nlam else lam, nlam)
                st = parity_stats(got.T, a.T, b.T, sun)
                print(f"{variant} | {frame} | {p} | {name} | canaries lost {lost} | " +
                      " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in st.items()), flush=True)

print("== 3. the sequence bake against the weighted sum of the per-frame references")
print("variant | frame | frames | image | ratio")
for variant in ("rgb", "spectral"):
    for rotated in (False, True):
        base = SC.base_dict(**({"to_world": SC.rotation()} if rotated else {}))
        em = ss.SunskyEmitter(base, variant)
        lam = SC.LAMBDAS if variant == "spectral" else None
        for count in (1, 3):
            suns = SC.frame_dirs(base.get("to_world"))[:count]
            seq = ss.SunskySequence(em, suns, SC.TURBIDITY[:count], SC.WEIGHTS[:count])
            for w, h in ((9, 7), (37, 13), (36, 9)):
                o64 = bound = 0.0
                for s, t, wt in zip(suns, SC.TURBIDITY, SC.WEIGHTS):
                    ref = R.BakeReference(variant, None, w, h, lam=lam, d=SC.frame_dict(base, s, t))
                    o64, bound = o64 + wt * ref.o64, bound + wt * ref.bound
                img = seq.bake_latlong(w, h, wavelengths=lam).cpu().numpy().reshape(-1, w * h)
                print(f"{variant} | {'rotated' if rotated else 'identity'} | {count} | {w}x{h} | "
                      f"{(np.abs(img - o64) / bound).max():.3f}", flush=True)
