"""The fp64 restatement of the samplers' disc term (tests/sampler_disc_reference.py) anchored to
the oracle, and its bound shown to have teeth, on host-only emitters:

* sky + mul S equals o64t's eval (the fp64 oracle after adopt_tables(em)) within 1e-12 on the disc
  lanes of every case of the GPU test, RGB and spectral;
* the fp32 reference, evaluated on its own sampled directions, exceeds bound() on most limb picks:
  a sampler no better than fp32 at the limb fails the GPU test.  The share asserted (>= 50 %) is
  for the default aperture at elevations >= 8 deg, where o32 is over a plain 1e-5 of o64t on
  95 % of the limb picks; at a lower sun the blue channel cancels, gamma_N A widens the bound and
  fewer fp32 lanes are outside it (printed), and at the wider apertures the figures are printed;
* the fp64 oracle on unrounded tables (o64) stays inside bound() at the default aperture: its
  distance to o64t is the table rounding (tests/test_oracle_table_modes.py).  Away from the
  default aperture o64's area ratio is the fp64 one, up to 2e-3 from the fp32 ratio the kernels
  and o64t take as given (oracle_adopt_tables), a scale of the whole disc term and not a rounding
  of its evaluation: printed there, not asserted.
Lanes where two oracles take different sides of the disc or horizon mask are left out of the
comparisons between them."""
import numpy as np
import pytest

import sampler_disc_reference as R
import sunsky_amd as ss

ALL = [c + (False,) for c in R.CASES] + [R.ROTATED + (True,)]


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
@pytest.mark.parametrize("elev,turb,aperture,rotated", ALL)
def test_restatement_anchor_and_bound_teeth(elev, turb, aperture, rotated, variant):
    d = R.case_dict(elev, turb, aperture, rotated=rotated)
    em = ss.SunskyEmitter(d, variant, precision="fast", device="host")
    o32, o64t, o64 = R.oracles(d, variant, em)
    u, limb = R.sun_pick_samples(em.sky_sampling_w, seed=int(elev * 10))
    lam = R.spectral_wavelengths(u.shape[0], seed=3) if variant == "spectral" else None
    s = o32.sample_direction(u, wavelengths=lam)
    gd, gp, w32 = s["d"], s["pdf"].astype(np.float64), s["weight"].astype(np.float64)
    disc = R.LocalDisc(em, aperture, to_local=R.TO_WORLD[:3, :3].T if rotated else None)
    tm = disc.terms(gd, lam)

    def ev(o):
        return o.eval(-gd, lam).T if lam is not None else o.eval(-gd)

    e32, e64t, e64 = ev(o32), ev(o64t), ev(o64)
    label = f"{variant} {elev} deg T {turb} ap {aperture}{' rotated' if rotated else ''}"

    # anchor: the same disc test and the same value as o64t
    hit = tm.hit
    assert hit.sum() > 15000, label
    nosun = ~hit
    assert np.array_equal(e64t[nosun] != 0, tm.eval[nosun] != 0)
    rel = np.abs(tm.eval - e64t)[hit] / np.maximum(np.abs(e64t[hit]), 1e-300)
    assert rel.max() <= 1e-12, f"{label}: restatement off o64t by {rel.max():.3e}"
    rel_sky = np.abs(tm.eval - e64t)[nosun] / np.maximum(np.abs(e64t[nosun]), 1e-300)
    assert rel_sky.size == 0 or rel_sky.max() <= 1e-12, label

    t = e64t / np.where(gp > 0, gp, 1.0)[:, None]
    bound = disc.bound(tm, t, gp)
    lanes = hit & (gp > 0) & ~R.disc_flip_lanes(e32, e64t)
    over32 = (np.abs(w32 - t) > bound).any(axis=1)
    plain32 = (np.abs(w32 - t) > R.RTOL * np.abs(t)).any(axis=1)
    share = over32[lanes & limb].mean()
    lanes64 = lanes & ~R.disc_flip_lanes(e64, e64t)
    r64 = (np.abs(e64 / np.where(gp > 0, gp, 1.0)[:, None] - t) / bound)[lanes64].max()
    print(f"{label}: anchor {rel.max():.1e}; {int((lanes & limb).sum())} limb / {int((lanes & ~limb).sum())} uniform "
          f"disc lanes; o32 over bound {share:.3f} of limb, {int(over32[lanes & ~limb].sum())} uniform; o32 over plain "
          f"1e-5: {int(plain32[lanes & limb].sum())} limb, {int(plain32[lanes & ~limb].sum())} uniform; "
          f"o64 worst {r64:.3f} x bound")
    assert (lanes & limb).sum() > 1000, label
    if aperture == 0.5358:
        assert r64 <= 1.0, f"{label}: o64 at {r64:.3f} x bound"
        if elev >= 8.0:
            assert share >= 0.5, f"{label}: o32 over bound on only {share:.3f} of the limb picks"
    assert over32[lanes & limb].any(), label


def test_sun_pick_samples_cover_the_square_edges():
    w = np.float32(0.3517)
    u, limb = R.sun_pick_samples(w, seed=1)
    assert u.shape == (R.N_UNIFORM + R.N_LIMB, 2) and limb.sum() == R.N_LIMB
    assert (u[:, 0] >= w).all() and (u < 1).all() and (u[:, 1] >= 0).all()   # every lane a sun pick
    a = (u[limb, 0].astype(np.float64) - w) / (1.0 - w)
    b = u[limb, 1].astype(np.float64)
    edge = np.minimum(np.minimum(a, 1 - a), np.minimum(b, 1 - b))
    assert edge.max() <= 1.0001e-4 + 1e-7
    k = R.N_UNIFORM
    one = np.nextafter(np.float32(1), np.float32(0))
    assert u[k, 0] == w and u[k + 1, 0] == np.nextafter(w, np.float32(1)) and u[k + 2, 0] == one
    assert u[k + 3, 1] == 0 and u[k + 4, 1] == one
    for e in ((a < 2e-4), (a > 1 - 2e-4), (b < 2e-4), (b > 1 - 2e-4)):
        assert e.sum() > 800
    lam = R.spectral_wavelengths(u.shape[0], seed=3)
    assert lam.min() >= 320 and lam.max() <= 720 and (lam[:, limb] == 720).any() and (lam[:, limb] == 360).any()
    nodes = np.arange(320, 721, 40, dtype=np.float32)
    assert all((lam[:, limb] == v).any() for v in nodes)
