"""fp64 restatement of the sun-disc term the FAST samplers add to a sun pick's weight, with the
condition sums that bound an fp32 evaluation of it (tests/test_sampler_disc_reference_cpu.py
anchors it to the oracle, tests/test_gpu_sampler_disc_literal.py holds the kernels to it).

Everything is read from the product's staged fp32 state: em.table("sun_radiance"), ("sun_ld"),
("sky_params"), ("sky_radiance"), em.info() (local sun direction n, cos_cutoff, the scales and
the fp32 area ratio) and the fp32 segment decision oracle.sun_segment_f32.  For a local
direction wo = (wx, wy, z) inside the disc (sunsky.cpp:572-614, 631-650, sunsky.h:385-392):

    x     = pi/2 - acos z - pi/2 (pos / 45)^3                pos = sun_segment_f32(z)
    gamma = 2 asin(|wo - n| / 2)                             unit_angle, sunsky.cpp:311
    c     = cos psi = sqrt(max(1 - sin^2 gamma / sin^2(aperture / 2), 0))
    RGB       S_ch = sum_kj x^k c^j T[pos][ch][k][j]          T: (45, 3, 4, 6), add_sun_rgb64
    spectral  S    = lerp(P_lo, P_hi, f) lerp-sum_j c^j (L[lo][j], L[hi][j], f)
              P_q  = sum_k x^k T[pos][q][k]                   T: (45, 11, 4), L: (11, 6), add_sun_spec64
              lo = floor((lambda - 320) / 40), f the remainder; channel 11 (f = 0 at 720 nm) is 0
    eval  = sky + mul S
    mul   = sun_scale area_ratio 467.069280386 / 106.7502593994140625 (RGB), sun_scale area_ratio
            (spectral): the folded multiplier of sunsky_model.cpp stage_geometry, in fp64 from the
            fp32 sun_scale and the fp32 area ratio the kernels take as given.

A is the same sum with every term's absolute value (spectral: the product of the two absolute
sums, the channel pair lerped with absolute values), dSdx and dSdc the partial derivatives in x
and cos psi, dSdf (spectral) the one in f.

bound(t, pdf): the admissible error of a FAST sampler's weight w = eval / pdf against
t = o64t.eval / pdf on a disc lane,

    rtol |t| + (gamma_N A + |dSdx| dx + |dSdc| dc + |dSdf| df) mul / pdf

  rtol = 1e-5, the project's bar: the sky value (1e-3 ... 1e-5 of the disc term), the addition
      to it, v_rcp_f32 of the pdf and the final product, all relative to the whole value.
  gamma_N = N u / (1 - N u), u = 2^-24: the forward bound of an fp32 sum of products in which
      no term passes more than N roundings (Higham, Accuracy and Stability, 3.1 / 5.1), against
      the absolute sum A.  N counted from sunsky_kernels.hip:
      RGB (render_sun_rgb_rows, render_sun_rgb_compact: the same nested Horner forms): 5 fmaf in
        cos psi, 4 fmaf in x, the product with K.sun_mul: 10; K.sun_mul itself is an fp32 product
        of four factors two of which (the conversion constants) are rounded to fp32 first: 5
        more roundings against the fp64 mul above.  N = 15.
      spectral (sun_powers + sun_spec_poly + lerpf_ + the limb-darkening sum of sun_spec_pair):
        x^3 2, three fmaf 3, the lerp 2 (fma(b, f, fma(-a, f, a)): each operand's share rounded
        at most twice, against |a| (1 - f) + |b| f) = 7 for the radiance; c^5 4, the coefficient
        lerp 2, six fmaf 6 = 12 for the limb darkening; the product of the two, the product with
        K.sun_mul and K.sun_mul's own rounding 3.  N = 22.  The rolled form the general kernel
        takes for other wavelength counts (sun_spec_term: render_sun_spec, sun_limb_darkening
        with powif_ products and separate adds) has one more in the limb darkening: N = 23 is
        used for both.
  dx: x = elevation_fast(z) - kHalfPi (frac frac frac), frac = pos (1 / 45), in fp32 against the
      fp64 x above on the same fp32 z: elevation_fast is within e ulp of the elevation E (an ulp
      is at most 2^-23 E), e = 0.71 up to its switch z = 0.70710678 (asin_half_chord's stated
      figure, 0.708 over every float on the GPU) and 4.11 above it, where it is pi/2 - 2 asin of
      a square root (the operation-count bound of tests/test_gpu_device_math.py; 2.16 measured:
      the 0.7 this term used to carry for every z does not hold there); the segment start
      B = pi/2 (pos / 45)^3 carries the rounding of 1 / 45, three products and kHalfPi and its
      product, 6 u B; the subtraction (or the fma's one rounding) u |x|.
      dx = e 2^-23 E + 6 u B + u |x|.
  dc: cos psi = v_sqrt_f32(max(c2, 0)) with c2 the fp32 rounding of an fp64 expression of the
      exact chord (the comment in add_sun_terms): relative u on c2 is u / 2 on c, the 1 ulp
      square root 2^-23 c.  The fp64 expression itself (cpsi_inv_hi + cpsi_inv_lo carries
      1 / sin^2 to 2^-48, a handful of fp64 roundings of numbers <= 1) is within e = 2^-46 of
      c^2 absolutely, which moves c by at most min(e / 2c, sqrt e).
      dc = 1.25 2^-23 c + min(2^-47 / c, 2^-23).
  df (spectral): f = nw - floor nw with nw = (lambda - 320) / 40 one correctly rounded fp32
      division of an exact difference (lambda in [360, 720]), so df = u nw; the remainder is
      exact.
  The derivative terms are first order; the second order is below 1e-13 of S (dc / c <= 2e-7
  wherever the first term of dc dominates).
No term in |o32 - o64|, no constant fitted to a kernel's output.

A rotated emitter: the kernels form wo = to_local(to_world(sd)) with fp32 dot products, the oracle
rotates in fp64.  LocalDisc takes the 3x3 to_local; the rotated case of the tests is a cyclic
permutation of the axes, whose products with 0 and 1 are exact in fp32, so no rounding of the
rotation enters and bound() stays as derived.
"""
import math

import numpy as np

import oracle as O

U = 2.0 ** -24
RTOL = 1e-5
ELEVATION_SWITCH = math.asin(float(np.float32(0.70710678)))   # elevation_fast changes form above this elevation
N_RGB = 15
N_SPEC = 23
SPEC_TO_RGB_SUN_CONV = 467.069280386
CIE_Y_NORMALIZATION = 1.0 / 106.7502593994140625

# (elevation deg, turbidity, aperture deg): tests/test_gpu_disc_literal.py CASES and EXTRA, and a
# 5 deg disc at 3 deg whose elevations span more than kSunRowsStaged = 8 segments
CASES = [(45.0, 2.0, 0.5358), (45.0, 10.0, 0.5358), (30.0, 3.0, 0.5358), (8.0, 6.0, 0.5358), (2.5, 1.5, 0.5358),
         (89.0, 3.0, 0.5358), (0.6, 4.0, 0.5358), (20.0, 2.5, 5.0), (60.0, 7.0, 12.0), (3.0, 3.0, 5.0)]
ROTATED = (30.0, 3.0, 0.5358)
TO_WORLD = np.array([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
N_UNIFORM, N_LIMB = 16384, 4096


def case_dict(elev, turb, aperture, albedo=0.2, rotated=False):
    th, phi = np.deg2rad(90.0 - elev), 0.3
    d = {"type": "sunsky", "sun_direction": [float(np.cos(phi) * np.sin(th)), float(np.sin(phi) * np.sin(th)),
                                             float(np.cos(th))],
         "sun_scale": 1.0, "sky_scale": 1.0, "turbidity": turb, "albedo": albedo, "sun_aperture": aperture}
    if rotated:
        d["to_world"] = TO_WORLD.copy()
    return d


def gamma_n(n):
    return n * U / (1.0 - n * U)


def sun_pick_samples(w_sky, seed):
    """(u (n, 2) fp32, limb (n,) bool): N_UNIFORM uniform sun picks, then N_LIMB picks whose cone
    sample ((u.x - w_sky) / (1 - w_sky), u.y) lies within 1e-4 rand of one of the four edges of
    the unit square, which the concentric warp maps to the limb.  The first limb lanes sit on the
    edges themselves: u.x = w_sky (a sun pick: the sky test is u.x < w_sky), the next float above
    it and 1 - ulp, u.y = 0 and 1 - ulp."""
    rng = np.random.default_rng(seed)
    w = np.float32(w_sky)
    one = np.nextafter(np.float32(1), np.float32(0))
    n = N_UNIFORM + N_LIMB
    s = rng.random((n, 2))
    edge = rng.integers(0, 4, N_LIMB)
    off = 1e-4 * rng.random(N_LIMB)
    lim = s[N_UNIFORM:]
    lim[edge == 0, 0] = off[edge == 0]
    lim[edge == 1, 0] = 1.0 - off[edge == 1]
    lim[edge == 2, 1] = off[edge == 2]
    lim[edge == 3, 1] = 1.0 - off[edge == 3]
    u = np.empty((n, 2), np.float32)
    u[:, 0] = (np.float64(w) + (1.0 - np.float64(w)) * s[:, 0]).astype(np.float32)
    u[:, 1] = s[:, 1].astype(np.float32)
    u[:, 0] = np.clip(u[:, 0], w, one)
    u[:, 1] = np.minimum(u[:, 1], one)
    k = N_UNIFORM
    u[k:k + 3, 0] = [w, np.nextafter(w, np.float32(1)), one]
    u[k + 3:k + 5, 1] = [0.0, one]
    limb = np.zeros(n, bool)
    limb[N_UNIFORM:] = True
    return u, limb


def spectral_wavelengths(n, seed):
    """(4, n) fp32: random in [360, 720], a block at the 11 nodes (320 and 720 included: 320 is
    outside the sampled range and evaluates like any node) and at 360 / 720."""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(360.0, 720.0, (4, n)).astype(np.float32)
    nodes = np.arange(320, 721, 40, dtype=np.float32)
    k = N_UNIFORM + 64   # inside the limb picks
    lam[:, k:k + 11 * 8] = np.tile(nodes, 8)[None, :]
    lam[0, k + 88:k + 120] = 360.0
    lam[1, k + 88:k + 120] = 720.0
    lam[:, :88] = np.tile(nodes, 8)[None, :]
    lam[2, 88:120] = 360.0
    lam[3, 88:120] = 720.0
    return lam


_asin, _acos, _sin = (np.vectorize(f, otypes=[np.float64]) for f in (math.asin, math.acos, math.sin))


class DiscTerms:
    """Per lane and channel (n, C): sky, S, A, dSdx, dSdc, dSdf (zeros for RGB); per lane: hit
    (inside the fp32-staged disc and above the horizon, decided in fp64 on the fp32 inputs as
    o64t does), x, c, E, B, nw (spectral, (n, C)); mul."""


class LocalDisc:
    def __init__(self, em, aperture_deg, to_local=None):
        inf = em.info()
        self.spectral = inf["nb_channels"] == 11
        self.n = np.asarray(inf["sun_dir_local"], np.float32).astype(np.float64)
        self.cos_cutoff = float(np.float32(inf["cos_cutoff"]))
        self.sky_scale = float(np.float32(inf["sky_scale"]))
        self.sun_scale, self.area_ratio = float(np.float32(inf["sun_scale"])), float(np.float32(inf["area_ratio"]))
        self.mul = self.sun_scale * self.area_ratio * ((SPEC_TO_RGB_SUN_CONV * CIE_Y_NORMALIZATION) if not self.spectral else 1.0)
        half = 0.5 * float(np.float32(aperture_deg)) * (math.pi / 180.0)
        self.inv_sin2 = 1.0 / (math.sin(half) * math.sin(half))
        nch = 11 if self.spectral else 3
        self.sky_params = em.table("sky_params").astype(np.float64).reshape(nch, 9)
        self.sky_rad = em.table("sky_radiance").astype(np.float64)
        sun = em.table("sun_radiance").astype(np.float64)
        self.sun = sun.reshape(45, 11, 4) if self.spectral else sun.reshape(45, 3, 4, 6)
        self.ld = em.table("sun_ld").astype(np.float64).reshape(11, 6)
        self.to_local = None if to_local is None else np.asarray(to_local, np.float64)
        self.n_rounds = N_SPEC if self.spectral else N_RGB

    def _sky(self, ch, z, gamma):
        k = np.moveaxis(self.sky_params[ch], -1, 0)   # (9, ...) broadcast over lanes
        cg = np.cos(gamma)
        cg2 = cg * cg
        c1 = 1 + k[0] * np.exp(k[1] / (z + 0.01))
        chi = (1 + cg2) / np.power(1 + k[8] * k[8] - 2 * k[8] * cg, 1.5)
        c2 = k[2] + k[3] * np.exp(k[4] * gamma) + k[5] * cg2 + k[6] * chi + k[7] * np.sqrt(np.maximum(z, 0))
        return c1 * c2 * self.sky_rad[ch]

    def terms(self, d, wavelengths=None, hit=None):
        """d: (n, 3) fp32 directions towards the sky (world); wavelengths (4, n) fp32, spectral.
        hit: the disc test's outcome per lane, to override the fp64 test on the fp32 inputs
        (the fp32 test's side on a lane where the two differ: next to the limb S continues with
        cos psi = 0)."""
        wo = np.asarray(d, np.float32).astype(np.float64)
        if self.to_local is not None:
            wo = wo @ self.to_local.T
        nl = wo.shape[0]
        z = wo[:, 2]
        dot = wo @ self.n
        sg = np.where(np.signbit(dot), -1.0, 1.0)
        v = wo - sg[:, None] * self.n
        half_chord = 0.5 * np.sqrt((v * v).sum(axis=1))
        temp = 2 * _asin(np.minimum(half_chord, 1.0))
        gamma = np.where(dot >= 0, temp, math.pi - temp)
        active = z >= 0
        t = DiscTerms()
        t.hit = active & ((dot >= self.cos_cutoff) if hit is None else np.asarray(hit, bool))
        t.E = 0.5 * math.pi - _acos(np.clip(z, -1.0, 1.0))
        pos = O.sun_segment_f32(z.astype(np.float32)).astype(np.int64)
        frac = pos / 45.0
        t.B = 0.5 * math.pi * (frac * frac * frac)
        t.x = t.E - t.B
        t.pos = pos
        sgam = _sin(gamma)
        t.c = np.sqrt(np.maximum(1.0 - self.inv_sin2 * sgam * sgam, 0.0))
        # powers by repeated products and sums in the oracle's term order (render_sun, sun_ld of
        # oracle_impl.inc), so that the anchor to o64t holds to rounding even where a channel cancels
        xk, cj = [np.ones(nl)], [np.ones(nl)]
        for _ in range(3):
            xk.append(xk[-1] * t.x)
        for _ in range(5):
            cj.append(cj[-1] * t.c)
        xk, cj = np.stack(xk, 1), np.stack(cj, 1)                                # (n, 4), (n, 6)
        dxk = np.stack([np.zeros(nl), np.ones(nl), 2 * t.x, 3 * xk[:, 2]], 1)
        dcj = np.stack([np.zeros(nl)] + [j * cj[:, j - 1] for j in range(1, 6)], 1)
        hit = t.hit[:, None]
        if not self.spectral:
            T = self.sun[pos]                                                   # (n, 3, 4, 6)
            S = np.zeros((nl, 3))
            for k in range(4):
                for j in range(6):
                    S += (xk[:, k] * cj[:, j])[:, None] * T[:, :, k, j]
            t.A = np.einsum("nckj,nk,nj->nc", np.abs(T), np.abs(xk), cj)
            t.dSdx = np.einsum("nckj,nk,nj->nc", T, dxk, cj)
            t.dSdc = np.einsum("nckj,nk,nj->nc", T, xk, dcj)
            t.dSdf = np.zeros_like(S)
            sky = self.sky_scale * np.stack([self._sky(c, z, gamma) for c in range(3)], 1) * CIE_Y_NORMALIZATION
            mul = self.mul
        else:
            lam = np.asarray(wavelengths, np.float32).astype(np.float64).T       # (n, 4)
            nw = (lam - 320.0) / 40.0
            valid = (nw >= 0) & (nw <= 10)
            lo = np.clip(np.floor(nw), 0, 10).astype(np.int64)
            hi = np.minimum(lo + 1, 10)
            f = np.where(valid, nw - lo, 0.0)
            has_hi = (lo + 1 < 11)[..., None]
            ii = pos[:, None]
            Tlo, Thi = self.sun[ii, lo], np.where(has_hi, self.sun[ii, hi], 0.0)    # (n, 4, 4)
            Llo, Lhi = self.ld[lo], np.where(has_hi, self.ld[hi], 0.0)            # (n, 4, 6)
            ff = f[..., None]
            Pl, Ph = np.zeros((nl, 4)), np.zeros((nl, 4))
            for k in range(4):
                Pl += xk[:, k, None] * Tlo[:, :, k]
                Ph += xk[:, k, None] * Thi[:, :, k]
            P = Ph * f + (-Pl * f + Pl)
            AP = np.einsum("nwk,nk->nw", (1 - ff) * np.abs(Tlo) + ff * np.abs(Thi), np.abs(xk))
            dP = np.einsum("nwk,nk->nw", Tlo + ff * (Thi - Tlo), dxk)
            Lf = Lhi * ff + (-Llo * ff + Llo)
            Ld = np.zeros((nl, 4))
            for j in range(6):
                Ld += cj[:, j, None] * Lf[:, :, j]
            ALd = np.einsum("nwj,nj->nw", (1 - ff) * np.abs(Llo) + ff * np.abs(Lhi), cj)
            dLd = np.einsum("nwj,nj->nw", Lf, dcj)
            S = P * Ld
            t.A = AP * ALd
            t.dSdx = dP * Ld
            t.dSdc = P * dLd
            t.dSdf = (Ph - Pl) * Ld + P * np.einsum("nwj,nj->nw", Lhi - Llo, cj)
            t.nw = nw
            zz, gg = z[:, None], gamma[:, None]
            a = self._sky(lo, zz, gg)
            b = np.where(has_hi[..., 0], self._sky(hi, zz, gg), 0.0)
            sky = self.sky_scale * (b * f + (-a * f + a))
            hit = hit & valid
            sky = np.where(valid, sky, 0.0)
            mul = self.mul
        t.S = np.where(hit, S, 0.0)
        for k in ("A", "dSdx", "dSdc", "dSdf"):
            setattr(t, k, np.where(hit, getattr(t, k), 0.0))
        t.sky = np.where(active[:, None], sky, 0.0)
        t.mul = mul
        if self.spectral:     # eval_local's own operation order (the folded mul differs by roundings only)
            t.eval = t.sky + self.sun_scale * t.S * self.area_ratio
        else:
            t.eval = (t.sky / CIE_Y_NORMALIZATION + self.sun_scale * t.S * self.area_ratio * SPEC_TO_RGB_SUN_CONV) \
                * CIE_Y_NORMALIZATION
        return t

    def bound(self, terms, ref, pdf):
        """(n, C): the admissible |w - ref| of a FAST sampler's weight on the disc lanes, for the
        reference weights ref (n, C) and the density pdf, (n,) or (n, C), the weights were divided by."""
        t = terms
        e = np.where(t.E > ELEVATION_SWITCH, 4.11, 0.71)   # elevation_fast below / above z = 0.70710678
        dx = e * 2.0 ** -23 * np.abs(t.E) + 6 * U * t.B + U * np.abs(t.x)
        dc = 1.25 * 2.0 ** -23 * t.c + np.minimum(2.0 ** -47 / np.maximum(t.c, 1e-300), 2.0 ** -23)
        err = gamma_n(self.n_rounds) * t.A + np.abs(t.dSdx) * dx[:, None] + np.abs(t.dSdc) * dc[:, None]
        if self.spectral:
            err = err + np.abs(t.dSdf) * (U * np.abs(t.nw))
        pdf = np.asarray(pdf, np.float64)
        pdf = pdf[:, None] if pdf.ndim == 1 else pdf
        scaled = np.where(pdf > 0, err * t.mul / np.where(pdf > 0, pdf, 1.0), 0.0)
        return RTOL * np.abs(ref) + scaled


def oracles(d, variant, em):
    """(o32, o64t, o64): the fp32 reference, the fp64 value of the product's staged fp32 state,
    and the fp64 oracle on unrounded tables; all three with the product's sampling state."""
    from helpers import fp32_sun_input
    o32 = O.Oracle(d, variant, "jit", "f32")
    d64 = fp32_sun_input(d, o32)
    o64 = O.Oracle(d64, variant, "jit", "f64")
    o64t = O.Oracle(d64, variant, "jit", "f64")
    o64t.adopt_tables(em)
    for o in (o32, o64t, o64):
        o.adopt_sampling_state(em)
    return o32, o64t, o64


def disc_flip_lanes(e32, e64t):
    """Lanes where o32 and o64t take different sides of the disc (or horizon) mask: helpers'
    mask_flip_lanes rule -- one value zero and the other not, or a factor above 2 between them --
    on the lane's largest channel.  The disc term is 1e2-1e6 times the sky on that channel, while
    a channel of a low sun's disc term can cross zero inside the disc (the RGB blue channel at
    3 deg: weights of -0.009 ... 0.06), where o32 and o64t differ by any factor on the same side
    of the mask."""
    a, b = np.abs(np.asarray(e32, np.float64)), np.abs(np.asarray(e64t, np.float64))
    m = np.argmax(np.maximum(a, b), axis=1)[:, None]
    ref = max(float(b.max()), 1e-30)
    am, bm = np.take_along_axis(a, m, 1)[:, 0], np.take_along_axis(b, m, 1)[:, 0]
    hi, lo = np.maximum(am, bm), np.minimum(am, bm)
    return (hi > 1e-6 * ref) & (hi - lo > 0.5 * hi)
