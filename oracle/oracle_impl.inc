/*
 * oracle_impl.inc -- TEST INFRASTRUCTURE ONLY (see sunsky_oracle.h).
 *
 * Precision-generic body, included twice by sunsky_oracle.c with
 *   R    = float  / double
 *   SFX  = f32    / f64
 *   F(x) = x##f   / x        (libm function selection)
 * Every function cites the reference file:line it restates.  Third-party
 * arithmetic (Dr.Jit 1.0.4, pyproject.toml:5, not vendored under
 * /root/reference) is restated from its published algorithms: unit_angle,
 * sphdir, lerp = fmadd(b,t,fnmadd(a,t,a)), Giles' erfinv.
 */

#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)
#define N_(name) CAT(name, CAT(_, SFX))
#define O_T CAT(oracle_, SFX)

typedef struct { R x, y, z; } N_(v3);
#define V3 N_(v3)

static const R N_(PI) = (R)3.14159265358979323846;
#define PI_ N_(PI)

static inline R N_(lerp)(R a, R b, R t) { return F(fma)(b, t, F(fma)(-a, t, a)); }
static inline R N_(safe_sqrt)(R x) { return F(sqrt)(x > 0 ? x : (R)0); }
static inline R N_(mulsign)(R a, R b) { return signbit(b) ? -a : a; }
static inline R N_(mulsign_neg)(R a, R b) { return signbit(b) ? a : -a; }
static inline R N_(powi)(R x, int k) { R r = 1; for (int i = 0; i < k; ++i) r *= x; return r; }
static inline R N_(dot)(V3 a, V3 b) { return F(fma)(a.z, b.z, F(fma)(a.y, b.y, a.x * b.x)); }
static inline R N_(norm)(V3 a) { return F(sqrt)(N_(dot)(a, a)); }
static inline R N_(clip)(R v, R lo, R hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* Dr.Jit unit_angle(a, b): numerically robust angle between unit vectors
   (used at sunsky.cpp:311, :812). */
static R N_(unit_angle)(V3 a, V3 b) {
    R d = N_(dot)(a, b);
    V3 v = { b.x - N_(mulsign)(a.x, d), b.y - N_(mulsign)(a.y, d), b.z - N_(mulsign)(a.z, d) };
    R temp = 2 * F(asin)((R)0.5 * N_(norm)(v));
    return d >= 0 ? temp : PI_ - temp;
}

/* Dr.Jit unit_angle_z(v) (sunsky.h:87, sunsky.cpp:835). */
static R N_(unit_angle_z)(V3 v) {
    R dz = v.z - N_(mulsign)((R)1, v.z);
    R temp = 2 * F(asin)((R)0.5 * F(sqrt)(F(fma)(v.x, v.x, F(fma)(v.y, v.y, dz * dz))));
    return v.z >= 0 ? temp : PI_ - temp;
}

/* from_spherical, sunsky.h:84-89: {atan2(y, x), unit_angle_z(v)} */
static void N_(from_spherical)(V3 v, R *phi, R *theta) {
    *phi = F(atan2)(v.y, v.x);
    *theta = N_(unit_angle_z)(v);
}

/* Dr.Jit sphdir(theta, phi) (sunsky.cpp:688, sunsky.h:373) */
static V3 N_(sphdir)(R theta, R phi) {
    R st = F(sin)(theta), ct = F(cos)(theta), sp = F(sin)(phi), cp = F(cos)(phi);
    V3 r = { cp * st, sp * st, ct };
    return r;
}

/* coordinate_system, vector.h:116-137 (Duff et al. 2017) */
static void N_(coordinate_system)(V3 n, V3 *s, V3 *t) {
    R sign = F(copysign)((R)1, n.z);
    R a = -1 / (sign + n.z);
    R b = n.x * n.y * a;
    s->x = N_(mulsign)(n.x * n.x * a, n.z) + 1;
    s->y = N_(mulsign)(b, n.z);
    s->z = N_(mulsign_neg)(n.x, n.z);
    t->x = b;
    t->y = F(fma)(n.y, n.y * a, sign);
    t->z = -n.y;
}

typedef struct { V3 s, t, n; } N_(frame);
#define FRAME N_(frame)

/* Frame::to_world, frame.h:36-38 */
static V3 N_(to_world)(const FRAME *f, V3 v) {
    V3 r;
    r.x = F(fma)(f->n.x, v.z, F(fma)(f->t.x, v.y, f->s.x * v.x));
    r.y = F(fma)(f->n.y, v.z, F(fma)(f->t.y, v.y, f->s.y * v.x));
    r.z = F(fma)(f->n.z, v.z, F(fma)(f->t.z, v.y, f->s.z * v.x));
    return r;
}

/* Transform::operator*(Vector), transform.h:149-158 (transform_affine on vectors) */
static V3 N_(xform_vec)(const R m[9], V3 v) {
    V3 r;
    r.x = F(fma)(m[2], v.z, F(fma)(m[1], v.y, m[0] * v.x));
    r.y = F(fma)(m[5], v.z, F(fma)(m[4], v.y, m[3] * v.x));
    r.z = F(fma)(m[8], v.z, F(fma)(m[7], v.y, m[6] * v.x));
    return r;
}

/* warp::square_to_uniform_disk_concentric, warp.h:54-90 */
static void N_(disk_concentric)(R sx, R sy, R *ox, R *oy) {
    R x = F(fma)((R)2, sx, (R)-1), y = F(fma)((R)2, sy, (R)-1);
    int is_zero = (x == 0) && (y == 0);
    int q13 = F(fabs)(x) < F(fabs)(y);
    R r = q13 ? y : x, rp = q13 ? x : y;
    R phi = (R)0.25 * PI_ * rp / r;
    if (q13) phi = (R)0.5 * PI_ - phi;
    if (is_zero) phi = 0;
    *ox = r * F(cos)(phi);
    *oy = r * F(sin)(phi);
}

/* warp::square_to_uniform_cone (approach 2), warp.h:533-551 */
static V3 N_(uniform_cone)(R sx, R sy, R cos_cutoff) {
    R omc = 1 - cos_cutoff, px, py;
    N_(disk_concentric)(sx, sy, &px, &py);
    R pn = F(fma)(px, px, py * py);
    R z = cos_cutoff + omc * (1 - pn);
    R sc = N_(safe_sqrt)(omc * (2 - omc * pn));
    V3 r = { px * sc, py * sc, z };
    return r;
}

/* gaussian_cdf, sunsky.h:113-115 */
static R N_(gaussian_cdf)(R mu, R sigma, R x) {
    const R inv_sqrt2 = (R)0.70710678118654752440;
    return (R)0.5 * (1 + F(erf)(inv_sqrt2 * (x - mu) / sigma));
}

/* erfinv: Dr.Jit restates M. Giles, "Approximating the erfinv function"
   (GPU Computing Gems, 2011), single-precision branch.  The fp64 instance
   polishes it with two Newton steps on erf so that it is the ideal value. */
static R N_(erfinv)(R x) {
    R w = -F(log)(F(fma)(x, -x, (R)1)), p;
    if (w < (R)5) {
        w = w - (R)2.5;
        p = (R)2.81022636e-08;
        p = F(fma)(p, w, (R)3.43273939e-07);
        p = F(fma)(p, w, (R)-3.5233877e-06);
        p = F(fma)(p, w, (R)-4.39150654e-06);
        p = F(fma)(p, w, (R)0.00021858087);
        p = F(fma)(p, w, (R)-0.00125372503);
        p = F(fma)(p, w, (R)-0.00417768164);
        p = F(fma)(p, w, (R)0.246640727);
        p = F(fma)(p, w, (R)1.50140941);
    } else {
        w = F(sqrt)(w) - (R)3;
        p = (R)-0.000200214257;
        p = F(fma)(p, w, (R)0.000100950558);
        p = F(fma)(p, w, (R)0.00134934322);
        p = F(fma)(p, w, (R)-0.00367342844);
        p = F(fma)(p, w, (R)0.00573950773);
        p = F(fma)(p, w, (R)-0.0076224613);
        p = F(fma)(p, w, (R)0.00943887047);
        p = F(fma)(p, w, (R)1.00167406);
        p = F(fma)(p, w, (R)2.83297682);
    }
    R y = p * x;
    if (sizeof(R) == 8) {
        for (int it = 0; it < 2; ++it) {
            R err = F(erf)(y) - x;
            y -= err / ((R)1.12837916709551257390 * F(exp)(-y * y));
        }
    }
    return y;
}

/* ------------------------------------------------------------------------ */
/* Emitter state                                                             */
/* ------------------------------------------------------------------------ */
struct O_T {
    oracle_params p;
    int spectral, nch, jit;
    /* datasets (fp64 file -> R, sunsky.cpp:182-199) */
    R *sky_params_ds, *sky_rad_ds, *sun_rad_ds, *sun_ld, *tgmm;
    R cie_y[11];
    /* staged */
    R to_world[9], to_local[9];
    V3 sun_dir_world, sun_dir_local;
    R sun_phi, sun_theta, sun_eta;
    FRAME frame;
    R half_aperture, cos_cutoff, area_ratio;
    R sky_params[11 * 9], sky_rad[11];
    R sun_rad[45 * 3 * 4 * 6]; /* max(RGB 3240, spectral 1980) */
    R gaussians[20 * 5], gauss_pmf[20], gauss_cdf[20], gauss_sum, gauss_norm;
    R w_sky;
    int spec_size;
    R spec_pdf[10], spec_cdf[9], spec_integral, spec_norm, spec_interval, spec_inv_interval;
    R bs_center[3], bs_radius;
    /* tables-as-staged mode (oracle_round_staged_tables / oracle_adopt_tables): render_sun
       takes the fp32 segment decision of the reference (sunsky.cpp:579-584) */
    int seg_f32;
};

/* compute_radiance_params + bezier_interpolate, sunsky.h:158-231 */
static void N_(compute_radiance_params)(const R *ds, int nch, int npar, const R *albedo,
                                         R turbidity, R eta, R *out) {
    static const R coefs[6] = { 1, 5, 10, 10, 5, 1 };
    const int result_size = nch * npar, a_block = 6 * result_size, t_block = 2 * a_block;
    R x = F(cbrt)(2 * ((R)1 / PI_) * eta);
    int t_high = (int)F(floor)(turbidity), t_low = t_high - 1;
    R t_rem = turbidity - (R)t_high;
    int in_range = (0 <= eta) && (eta <= (R)0.5 * PI_);
    for (int e = 0; e < result_size; ++e) {
        R bez[2][2]; /* [t low/high][albedo] */
        for (int ti = 0; ti < 2; ++ti) {
            int t = ti ? t_high : t_low;
            for (int a = 0; a < 2; ++a) {
                R res = 0;
                if (t >= 0 && t < 10) {
                    for (int k = 0; k < 6; ++k) {
                        R data = ds[t * t_block + a * a_block + k * result_size + e];
                        res += coefs[k] * N_(powi)(x, k) * N_(powi)(1 - x, 5 - k) * data;
                    }
                }
                bez[ti][a] = res;
            }
        }
        R ra_low = N_(lerp)(bez[0][0], bez[1][0], t_rem);
        R ra_high = N_(lerp)(bez[0][1], bez[1][1], t_rem);
        R v = N_(lerp)(ra_low, ra_high, albedo[e / npar]);
        out[e] = in_range ? v : (R)0;
    }
}

/* compute_sun_params, sunsky.h:404-419 */
static void N_(compute_sun_params)(const R *ds, int block, R turbidity, R *out) {
    int t_high = (int)F(floor)(turbidity), t_low = t_high - 1;
    R t_rem = turbidity - (R)t_high;
    for (int i = 0; i < block; ++i) {
        R lo = (t_low >= 0 && t_low < 10) ? ds[t_low * block + i] : (R)0;
        R hi = (t_high >= 0 && t_high < 10) ? ds[t_high * block + i] : (R)0;
        out[i] = N_(lerp)(lo, hi, t_rem);
    }
}

/* compute_tgmm_distribution, sunsky.h:438-501 */
static void N_(compute_tgmm)(const R *tables, R turbidity, R eta, R *params, R *weights) {
    R eta_deg = eta * (R)(180.0 / 3.14159265358979323846);
    R eta_idx_f = N_(clip)((eta_deg - 2) / 3, 0, 29), t_idx_f = N_(clip)(turbidity - 2, 0, 8);
    int eta_lo = (int)F(floor)(eta_idx_f), t_lo = (int)F(floor)(t_idx_f);
    int eta_hi = eta_lo + 1 < 29 ? eta_lo + 1 : 29, t_hi = t_lo + 1 < 8 ? t_lo + 1 : 8;
    R eta_rem = eta_idx_f - (R)eta_lo, t_rem = t_idx_f - (R)t_lo;
    const int result_size = 25, t_block = 30 * result_size;
    int idx[4] = { t_lo * t_block + eta_lo * result_size, t_lo * t_block + eta_hi * result_size,
                   t_hi * t_block + eta_lo * result_size, t_hi * t_block + eta_hi * result_size };
    R lf[4] = { (1 - t_rem) * (1 - eta_rem), (1 - t_rem) * eta_rem, t_rem * (1 - eta_rem),
                t_rem * eta_rem };
    for (int m = 0; m < 4; ++m)
        for (int i = 0; i < result_size; ++i) {
            R v = tables[idx[m] + i];
            if (i % 5 == 4) v = v * lf[m];
            params[m * result_size + i] = v;
        }
    for (int g = 0; g < 20; ++g) weights[g] = params[g * 5 + 4];
}

/* render_sky, sunsky.cpp:538-555 */
static R N_(render_sky)(const O_T *o, int c, R cos_theta, R gamma) {
    const R *k = o->sky_params + c * 9;
    R cg = F(cos)(gamma), cg2 = cg * cg;
    R c1 = 1 + k[0] * F(exp)(k[1] / (cos_theta + (R)0.01));
    R chi = (1 + cg2) / F(pow)(1 + k[8] * k[8] - 2 * k[8] * cg, (R)1.5);
    R c2 = k[2] + k[3] * F(exp)(k[4] * gamma) + k[5] * cg2 + k[6] * chi + k[7] * N_(safe_sqrt)(cos_theta);
    return c1 * c2 * o->sky_rad[c];
}

/* compute_cos_psi, sunsky.h:385-392 */
static R N_(cos_psi)(R gamma, R half_aperture) {
    R s = F(sin)(half_aperture), ar2 = 1 / (s * s), sg = F(sin)(gamma);
    R sc2 = (R)1.0 - ar2 * sg * sg;
    return N_(safe_sqrt)(sc2);
}

/* render_sun's segment search, sunsky.cpp:579-584 */
static int N_(sun_segment)(R cos_theta) {
    R elevation = (R)0.5 * PI_ - F(acos)(cos_theta);
    R seg = F(cbrt)(2 * elevation * ((R)1 / PI_)) * 45;
    int pos = (int)F(floor)(seg);
    if (seg < 0) pos = 0; /* floor2int<UInt32> of a tiny negative: never hit for cos_theta >= 0 */
    if (pos > 44) pos = 44;
    return pos;
}

int CAT(oracle_sun_segment_, SFX)(R cos_theta) { return N_(sun_segment)(cos_theta); }

/* render_sun, sunsky.cpp:572-614 */
static R N_(render_sun)(const O_T *o, int c, R cos_theta, R gamma) {
    R elevation = (R)0.5 * PI_ - F(acos)(cos_theta);
    int pos = o->seg_f32 ? oracle_sun_segment_f32((float)cos_theta) : N_(sun_segment)(cos_theta);
    R frac = (R)pos / 45;
    R break_x = (R)0.5 * PI_ * (frac * frac * frac);
    R x = elevation - break_x;
    R res = 0;
    if (o->spectral) {
        const R *s = o->sun_rad + pos * 11 * 4 + c * 4;
        for (int k = 0; k < 4; ++k) res += N_(powi)(x, k) * s[k];
    } else {
        R cp = N_(cos_psi)(gamma, o->half_aperture);
        const R *s = o->sun_rad + pos * (3 * 4 * 6) + c * (4 * 6);
        for (int k = 0; k < 4; ++k)
            for (int j = 0; j < 6; ++j)
                res += N_(powi)(x, k) * N_(powi)(cp, j) * s[k * 6 + j];
    }
    return res;
}

/* compute_sun_ld, sunsky.cpp:631-650 */
static R N_(sun_ld)(const O_T *o, int lo, int hi, R f, R gamma) {
    R cp = N_(cos_psi)(gamma, o->half_aperture), res = 0;
    for (int j = 0; j < 6; ++j) {
        R a = o->sun_ld[lo * 6 + j];
        R b = (hi < 11) ? o->sun_ld[hi * 6 + j] : (R)0;
        R coef = (f == 0) ? a : N_(lerp)(a, b, f);
        res += N_(powi)(cp, j) * coef;
    }
    return res;
}

/* SunskyEmitter::eval, sunsky.cpp:303-352, for one local direction.
   lambda ignored for RGB; out has 3 (RGB) or 1 (one wavelength) entries. */
static void N_(eval_local)(const O_T *o, V3 wo, R lambda, R *out) {
    R cos_theta = wo.z;
    R gamma = N_(unit_angle)(o->frame.n, wo);
    int active = cos_theta >= 0;
    int hit_sun = active && (N_(dot)(o->frame.n, wo) >= o->cos_cutoff);
    if (!o->spectral) {
        const R cie_norm = (R)(1.0 / 106.7502593994140625);
        const R conv = (R)467.069280386;
        for (int c = 0; c < 3; ++c) {
            R res = active ? o->p.sky_scale * N_(render_sky)(o, c, cos_theta, gamma) : (R)0;
            R sun = hit_sun ? N_(render_sun)(o, c, cos_theta, gamma) : (R)0;
            res += (R)o->p.sun_scale * sun * o->area_ratio * conv;
            res *= cie_norm;
            out[c] = active ? res : (R)0;
        }
    } else {
        R nw = (lambda - (R)320) / (R)40;
        int valid = ((R)0 <= nw) && (nw <= (R)10);
        int lo = (int)F(floor)(nw), hi = lo + 1;
        R f = nw - (R)lo;
        R res = 0;
        if (active && valid) {
            R a = N_(render_sky)(o, lo, cos_theta, gamma);
            R b = (f != 0 && hi < 11) ? N_(render_sky)(o, hi, cos_theta, gamma) : (R)0;
            res = o->p.sky_scale * ((f == 0) ? a : N_(lerp)(a, b, f));
        }
        if (hit_sun && valid) {
            R a = N_(render_sun)(o, lo, cos_theta, gamma);
            R b = (f != 0 && hi < 11) ? N_(render_sun)(o, hi, cos_theta, gamma) : (R)0;
            R sun = (f == 0) ? a : N_(lerp)(a, b, f);
            R ld = N_(sun_ld)(o, lo, hi, f, gamma);
            res += o->p.sun_scale * sun * ld * o->area_ratio;
        }
        out[0] = active ? res : (R)0;
    }
}

/* DiscreteDistribution::sample_reuse (distr_1d.h:173-183) with the JIT
   predicate of distr_1d.h:116-136, or the scalar bounds of :233-265. */
static int N_(discrete_sample)(const O_T *o, R value, R *reused) {
    R s = value * o->gauss_sum;
    int idx = 0;
    if (o->jit) {
        for (int i = 0; i < 19; ++i) {
            R c = o->gauss_cdf[i];
            if (((c < s) || c == 0) && c != o->gauss_sum) idx = i + 1; else break;
        }
    } else {
        int first = -1, last = -1;
        for (int i = 0; i < 20; ++i) if (o->gauss_pmf[i] > 0) { if (first < 0) first = i; last = i; }
        idx = first;
        while (idx < last && o->gauss_cdf[idx] < s) ++idx;
    }
    R pmf = o->gauss_pmf[idx] * o->gauss_norm;
    R cdf = idx > 0 ? o->gauss_cdf[idx - 1] * o->gauss_norm : (R)0;
    *reused = (value - cdf) / pmf;
    return idx;
}

/* sample_sky, sunsky.cpp:661-689 */
static V3 N_(sample_sky)(const O_T *o, R ux, R uy) {
    R temp;
    int idx = N_(discrete_sample)(o, ux, &temp);
    const R *g = o->gaussians + idx * 5;
    R mu_phi = g[0], mu_theta = g[1], s_phi = g[2], s_theta = g[3];
    R ca_x = N_(gaussian_cdf)(mu_phi, s_phi, 0), ca_y = N_(gaussian_cdf)(mu_theta, s_theta, 0);
    R cb_x = N_(gaussian_cdf)(mu_phi, s_phi, 2 * PI_), cb_y = N_(gaussian_cdf)(mu_theta, s_theta, (R)0.5 * PI_);
    R sx = N_(lerp)(ca_x, cb_x, temp), sy = N_(lerp)(ca_y, cb_y, uy);
    const R eps = (R)5.9604644775390625e-08, ome = (R)1 - (R)5.9604644775390625e-08;
    sx = N_(clip)(sx, eps, ome);
    sy = N_(clip)(sy, eps, ome);
    const R sqrt2 = (R)1.41421356237309504880;
    R phi = sqrt2 * N_(erfinv)(2 * sx - 1) * s_phi + mu_phi;
    R theta = sqrt2 * N_(erfinv)(2 * sy - 1) * s_theta + mu_theta;
    phi += o->sun_phi - (R)0.5 * PI_;
    R tmax = (R)0.5 * PI_ - eps;
    theta = theta < tmax ? theta : tmax;
    return N_(sphdir)(theta, phi);
}

/* sample_sun, sunsky.cpp:697-701 */
static V3 N_(sample_sun)(const O_T *o, R ux, R uy) {
    return N_(to_world)(&o->frame, N_(uniform_cone)(ux, uy, o->cos_cutoff));
}

/* tgmm_pdf, sunsky.cpp:732-763 */
static R N_(tgmm_pdf)(const O_T *o, R phi, R theta, int active) {
    phi -= o->sun_phi - (R)0.5 * PI_;
    if (phi < 0) phi += 2 * PI_;
    if (phi > 2 * PI_) phi -= 2 * PI_;
    active = active && (theta >= 0) && (theta <= (R)0.5 * PI_);
    R pdf = 0;
    const R inv_two_pi = (R)0.15915494309189533577;
    for (int i = 0; i < 20; ++i) {
        const R *g = o->gaussians + i * 5;
        R ca_x = N_(gaussian_cdf)(g[0], g[2], 0), ca_y = N_(gaussian_cdf)(g[1], g[3], 0);
        R cb_x = N_(gaussian_cdf)(g[0], g[2], 2 * PI_), cb_y = N_(gaussian_cdf)(g[1], g[3], (R)0.5 * PI_);
        R volume = (cb_x - ca_x) * (cb_y - ca_y) * (g[2] * g[3]);
        R sx = (phi - g[0]) / g[2], sy = (theta - g[1]) / g[3];
        R gp = inv_two_pi * F(exp)((R)-0.5 * F(fma)(sy, sy, sx * sx));
        pdf += g[4] * gp / volume;
    }
    return active ? pdf : (R)0;
}

/* compute_pdfs, sunsky.cpp:711-723 */
static void N_(compute_pdfs)(const O_T *o, V3 d, int check_sun, int active, R *sky_pdf, R *sun_pdf) {
    R sin_theta = N_(safe_sqrt)(F(fma)(d.x, d.x, d.y * d.y));
    active = active && (d.z >= 0) && (sin_theta != 0);
    const R sin_offset = (R)5.9604644775390625e-08;
    sin_theta = sin_theta > sin_offset ? sin_theta : sin_offset;
    R phi, theta;
    N_(from_spherical)(d, &phi, &theta);
    *sky_pdf = N_(tgmm_pdf)(o, phi, theta, active) / sin_theta;
    R sp = ((R)0.15915494309189533577) / (1 - o->cos_cutoff);
    *sun_pdf = (!check_sun || N_(dot)(o->frame.n, d) >= o->cos_cutoff) ? sp : (R)0;
}

/* ContinuousDistribution::sample_pdf, distr_1d.h:468-499 (JIT predicate) */
static R N_(cont_sample_pdf)(const O_T *o, R sample, R *pdf_out) {
    sample *= o->spec_integral;
    int nint = o->spec_size - 1, idx = 0;
    if (o->jit) {
        for (int i = 0; i < nint - 1; ++i) {
            R c = o->spec_cdf[i];
            if (((c < sample) || c == 0) && c != o->spec_integral) idx = i + 1; else break;
        }
    } else {
        while (idx < nint - 1 && o->spec_cdf[idx] < sample) ++idx;
    }
    R y0 = o->spec_pdf[idx], y1 = o->spec_pdf[idx + 1];
    R c0 = idx > 0 ? o->spec_cdf[idx - 1] : (R)0;
    sample = (sample - c0) * o->spec_inv_interval;
    R t_linear = (y0 - N_(safe_sqrt)(F(fma)(y0, y0, 2 * sample * (y1 - y0)))) * ((R)1 / (y0 - y1));
    R t_const = sample * ((R)1 / y0);
    R t = (y0 == y1) ? t_const : t_linear;
    *pdf_out = F(fma)(t, y1 - y0, y0) * o->spec_norm;
    return F(fma)((R)idx + t, o->spec_interval, (R)360);
}

/* estimate_sky_sun_ratio, sunsky.cpp:772-886 */
static void N_(estimate_sky_sun_ratio)(O_T *o) {
    if (!o->jit) {
        o->w_sky = (R)0.5;
        o->spec_size = 2;
        o->spec_pdf[0] = o->spec_pdf[1] = 1;
        return;
    }
    enum { NQ = 200 };
    double xd[NQ], wd[NQ];
    oracle_gauss_legendre(NQ, xd, wd);
    R x[NQ], w[NQ];
    for (int i = 0; i < NQ; ++i) { x[i] = (R)(float)xd[i]; w[i] = (R)(float)wd[i]; }
    /* nodes are ScalarFloat = fp32 in float variants: round through float */
    const int nch = o->nch;
    R sky[11] = { 0 }, sun[11] = { 0 };
    /* sky over the hemisphere */
    {
        R J = (R)0.5 * PI_;
        for (int c = 0; c < nch; ++c) {
            R acc = 0;
            double acc_x = 0;                    /* exact sum of the R terms (g_quad_sum_sequential = 0) */
            for (int j = 0; j < NQ; ++j) {        /* cos_theta index (meshgrid y) */
                R cos_theta = (R)0.5 * (x[j] + 1);
                R sin_theta = N_(safe_sqrt)(1 - cos_theta * cos_theta);
                for (int i = 0; i < NQ; ++i) {    /* phi index (meshgrid x) */
                    R phi = PI_ * (x[i] + 1);
                    V3 wo = { sin_theta * F(cos)(phi), sin_theta * F(sin)(phi), cos_theta };
                    R gamma = N_(unit_angle)(o->frame.n, wo);
                    R v = N_(render_sky)(o, c, cos_theta, gamma) * w[i] * w[j];
                    acc += v;
                    acc_x += (double)v;
                }
            }
            sky[c] = (g_quad_sum_sequential ? acc : (R)acc_x) * J;
        }
    }
    /* sun over its cone */
    {
        R cc = o->cos_cutoff;
        R J = (R)0.5 * PI_ * (1 - cc);
        for (int c = 0; c < nch; ++c) {
            R acc = 0;
            double acc_x = 0;
            for (int j = 0; j < NQ; ++j) {
                R cos_gamma = (R)0.5 * ((1 - cc) * x[j] + (1 + cc));
                R sin_gamma = N_(safe_sqrt)(1 - cos_gamma * cos_gamma);
                for (int i = 0; i < NQ; ++i) {
                    R phi = PI_ * (x[i] + 1);
                    V3 sw = { sin_gamma * F(cos)(phi), sin_gamma * F(sin)(phi), cos_gamma };
                    R gamma = N_(unit_angle_z)(sw);
                    V3 wl = N_(to_world)(&o->frame, sw);
                    R cos_theta = wl.z;
                    if (!(cos_theta >= 0)) continue;
                    R v = N_(render_sun)(o, c, cos_theta, gamma) * w[i] * w[j];
                    if (o->spectral) v *= N_(sun_ld)(o, c, c, 0, gamma);
                    acc += v;
                    acc_x += (double)v;
                }
            }
            sun[c] = (g_quad_sum_sequential ? acc : (R)acc_x) * J;
        }
    }
    R sky_lum = o->p.sky_scale, sun_lum = o->p.sun_scale;
    if (!o->spectral) {
        sky_lum *= sky[0] * (R)0.212671f + sky[1] * (R)0.715160f + sky[2] * (R)0.072169f;
        sun_lum *= (sun[0] * (R)0.212671f + sun[1] * (R)0.715160f + sun[2] * (R)0.072169f) *
                   o->area_ratio * (R)467.069280386;
    } else {
        R ls = 0, lu = 0;
        for (int c = 0; c < 11; ++c) { ls += o->cie_y[c] * sky[c]; lu += o->cie_y[c] * sun[c]; }
        sky_lum *= ls / 11;
        sun_lum *= lu / 11 * o->area_ratio;
    }
    R res = sky_lum / (sky_lum + sun_lum);
    if (res != res) res = 0;
    o->w_sky = res;
    if (o->spectral) {
        o->spec_size = 10;
        int all_zero = 1;
        for (int i = 0; i < 10; ++i) {
            o->spec_pdf[i] = sun[i + 1] + sky[i + 1];
            if (o->spec_pdf[i] != 0) all_zero = 0;
        }
        if (all_zero) for (int i = 0; i < 10; ++i) o->spec_pdf[i] += 1;
    } else {
        o->spec_size = 0;
    }
}

/* ContinuousDistribution::compute_cdf (JIT, distr_1d.h:513-538) /
   compute_cdf_scalar (:541-585) */
static void N_(build_spectral_distr)(O_T *o) {
    if (o->spec_size < 2) return;
    int size = o->spec_size;
    if (o->jit) {
        R interval = (R)(720 - 360) / (R)(size - 1);
        R prefix = 0, prefix_all[10];
        for (int i = 0; i < size; ++i) { prefix += o->spec_pdf[i]; prefix_all[i] = prefix; }
        for (int i = 1; i < size; ++i)
            o->spec_cdf[i - 1] = interval * (prefix_all[i] - (R)0.5 * o->spec_pdf[0] - (R)0.5 * o->spec_pdf[i]);
        o->spec_interval = interval;
    } else {
        double interval = (720.0 - 360.0) / (size - 1), integral = 0;
        for (int i = 0; i < size - 1; ++i) {
            integral += 0.5 * interval * ((double)o->spec_pdf[i] + (double)o->spec_pdf[i + 1]);
            o->spec_cdf[i] = (R)(float)integral;
        }
        o->spec_interval = (R)interval;
    }
    o->spec_integral = o->spec_cdf[size - 2];
    o->spec_norm = (R)1 / o->spec_integral;
    o->spec_inv_interval = (R)1 / o->spec_interval;
}

static R *N_(load_table)(const pack_file *pk, const char *name, size_t expect) {
    size_t n = 0;
    const void *src = pack_find(pk, name, &n);
    if (!src || n != expect) {
        set_error("oracle: pack entry '%s' missing or has %zu elements (expected %zu)", name, n, expect);
        return NULL;
    }
    R *dst = (R *)malloc(sizeof(R) * n);
    int dt = pack_dtype(pk, name);
    for (size_t i = 0; i < n; ++i) {
        double v = dt == 2 ? ((const double *)src)[i] : (double)((const float *)src)[i];
        dst[i] = sizeof(R) == 4 ? (R)(float)v : (R)v;
    }
    return dst;
}

/* SunskyEmitter ctor + init_from_props + parameters_changed (sunsky.cpp:162-218, 889-948) */
int N_(oracle_create)(const oracle_params *p, const char *pack_path, O_T **out) {
    *out = NULL;
    if (p->sun_scale < 0) { set_error("Invalid sun scale: %f, must be positive!", p->sun_scale); return 1; }
    if (p->sky_scale < 0) { set_error("Invalid sky scale: %f, must be positive!", p->sky_scale); return 1; }
    if (p->turbidity < 1 || 10 < p->turbidity) { set_error("Turbidity value %f is out of range [1, 10]", p->turbidity); return 1; }
    float half_ap = (float)(0.5f * p->sun_aperture_deg) * (float)(3.14159265358979323846 / 180.0);
    if (half_ap <= 0 || 0.5f * 3.14159265f <= half_ap) { set_error("Invalid sun aperture angle"); return 1; }
    pack_file pk;
    if (pack_open(&pk, pack_path)) return 1;
    O_T *o = (O_T *)calloc(1, sizeof(O_T));
    o->p = *p;
    o->spectral = p->spectral;
    o->nch = p->spectral ? 11 : 3;
    o->jit = p->jit_semantics;
    int ok = 1;
    if (o->spectral) {
        ok &= !!(o->sky_params_ds = N_(load_table)(&pk, "sky_spec_params", 10 * 2 * 6 * 11 * 9));
        ok &= !!(o->sky_rad_ds = N_(load_table)(&pk, "sky_spec_rad", 10 * 2 * 6 * 11));
        ok &= !!(o->sun_rad_ds = N_(load_table)(&pk, "sun_spec_rad", 10 * 45 * 11 * 4));
    } else {
        ok &= !!(o->sky_params_ds = N_(load_table)(&pk, "sky_rgb_params", 10 * 2 * 6 * 3 * 9));
        ok &= !!(o->sky_rad_ds = N_(load_table)(&pk, "sky_rgb_rad", 10 * 2 * 6 * 3));
        ok &= !!(o->sun_rad_ds = N_(load_table)(&pk, "sun_rgb_rad", 10 * 45 * 3 * 4 * 6));
    }
    ok &= !!(o->sun_ld = N_(load_table)(&pk, "sun_spec_ld", 11 * 6));
    ok &= !!(o->tgmm = N_(load_table)(&pk, "tgmm_tables", 9 * 30 * 5 * 5));
    R *cie = N_(load_table)(&pk, "cie_y_nodes", 11);
    ok &= !!cie;
    pack_close(&pk);
    if (!ok) { N_(oracle_destroy)(o); free(cie); return 1; }
    memcpy(o->cie_y, cie, sizeof(o->cie_y));
    free(cie);

    /* albedo per channel (extract_albedo, sunsky.cpp:956-978) */
    R albedo[11];
    for (int c = 0; c < o->nch; ++c) {
        float a = p->albedo_n == 1 ? p->albedo[0] : p->albedo[c];
        if (a < 0 || a > 1) { set_error("Albedo values must be in [0, 1], got: %f", a); N_(oracle_destroy)(o); return 1; }
        albedo[c] = (R)a;
    }

    /* to_world / inverse (Transform, transform.h:77-79; inverse computed in fp64) */
    double m[9], inv[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m[r * 3 + c] = p->to_world[r * 4 + c];
    double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    inv[0] = (m[4] * m[8] - m[5] * m[7]) / det; inv[1] = (m[2] * m[7] - m[1] * m[8]) / det; inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    inv[3] = (m[5] * m[6] - m[3] * m[8]) / det; inv[4] = (m[0] * m[8] - m[2] * m[6]) / det; inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    inv[6] = (m[3] * m[7] - m[4] * m[6]) / det; inv[7] = (m[1] * m[6] - m[0] * m[7]) / det; inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    for (int i = 0; i < 9; ++i) {
        o->to_world[i] = sizeof(R) == 4 ? (R)(float)m[i] : (R)m[i];
        o->to_local[i] = sizeof(R) == 4 ? (R)(float)inv[i] : (R)inv[i];
    }

    /* sun direction (init_from_props :912-946, ctor :174) */
    V3 sw;
    if (p->use_sun_direction) {
        V3 d = { p->sun_direction[0], p->sun_direction[1], p->sun_direction[2] };
        R inv_n = (R)1 / N_(norm)(d);
        sw.x = d.x * inv_n; sw.y = d.y * inv_n; sw.z = d.z * inv_n;
    } else {
        float s[3];
        oracle_sun_coordinates(p->year, p->month, p->day, p->hour, p->minute, p->second,
                               p->latitude, p->longitude, p->timezone, s);
        V3 loc = { s[0], s[1], s[2] };
        sw = N_(xform_vec)(o->to_world, loc);
    }
    o->sun_dir_world = sw;
    o->sun_dir_local = N_(xform_vec)(o->to_local, sw);
    N_(from_spherical)(o->sun_dir_local, &o->sun_phi, &o->sun_theta);
    o->frame.n = o->sun_dir_local;
    N_(coordinate_system)(o->frame.n, &o->frame.s, &o->frame.t);
    o->sun_eta = (R)0.5 * PI_ - o->sun_theta;

    o->half_aperture = sizeof(R) == 4 ? (R)half_ap
                       : (R)(0.5 * (double)p->sun_aperture_deg * (3.14159265358979323846 / 180.0));
    o->cos_cutoff = F(cos)(o->half_aperture);
    /* get_area_ratio, sunsky.h:99-101: SUN_HALF_APERTURE is a double expression */
    R ref_half = (R)(0.5358 / 2.0 * (3.14159265358979323846 / 180.0));
    o->area_ratio = (1 - F(cos)(ref_half)) / (1 - F(cos)(o->half_aperture));

    N_(compute_radiance_params)(o->sky_params_ds, o->nch, 9, albedo, (R)p->turbidity, o->sun_eta, o->sky_params);
    N_(compute_radiance_params)(o->sky_rad_ds, o->nch, 1, albedo, (R)p->turbidity, o->sun_eta, o->sky_rad);
    int sun_block = o->spectral ? 45 * 11 * 4 : 45 * 3 * 4 * 6;
    N_(compute_sun_params)(o->sun_rad_ds, sun_block, (R)p->turbidity, o->sun_rad);

    N_(compute_tgmm)(o->tgmm, (R)p->turbidity, o->sun_eta, o->gaussians, o->gauss_pmf);
    /* DiscreteDistribution cdf: JIT prefix_sum in fp32 (distr_1d.h:218-231),
       scalar accumulates in double (:233-265) */
    if (o->jit) {
        R acc = 0;
        for (int i = 0; i < 20; ++i) { acc += o->gauss_pmf[i]; o->gauss_cdf[i] = acc; }
    } else {
        double acc = 0;
        for (int i = 0; i < 20; ++i) { acc += (double)o->gauss_pmf[i]; o->gauss_cdf[i] = sizeof(R) == 4 ? (R)(float)acc : (R)acc; }
    }
    o->gauss_sum = o->gauss_cdf[19];
    o->gauss_norm = (R)1 / o->gauss_sum;

    N_(estimate_sky_sun_ratio)(o);
    N_(build_spectral_distr)(o);

    o->bs_center[0] = p->bsphere_center[0];
    o->bs_center[1] = p->bsphere_center[1];
    o->bs_center[2] = p->bsphere_center[2];
    o->bs_radius = p->bsphere_radius > 0 ? p->bsphere_radius : (R)1;
    *out = o;
    return 0;
}

void N_(oracle_destroy)(O_T *o) {
    if (!o) return;
    free(o->sky_params_ds); free(o->sky_rad_ds); free(o->sun_rad_ds);
    free(o->sun_ld); free(o->tgmm);
    free(o);
}

void N_(oracle_info)(const O_T *o, oracle_info *info) {
    memset(info, 0, sizeof(*info));
    info->sun_dir_world[0] = o->sun_dir_world.x; info->sun_dir_world[1] = o->sun_dir_world.y; info->sun_dir_world[2] = o->sun_dir_world.z;
    info->sun_dir_local[0] = o->sun_dir_local.x; info->sun_dir_local[1] = o->sun_dir_local.y; info->sun_dir_local[2] = o->sun_dir_local.z;
    info->sun_angles[0] = o->sun_phi; info->sun_angles[1] = o->sun_theta;
    info->frame_s[0] = o->frame.s.x; info->frame_s[1] = o->frame.s.y; info->frame_s[2] = o->frame.s.z;
    info->frame_t[0] = o->frame.t.x; info->frame_t[1] = o->frame.t.y; info->frame_t[2] = o->frame.t.z;
    info->sun_eta = o->sun_eta; info->w_sky = o->w_sky; info->area_ratio = o->area_ratio;
    info->cos_cutoff = o->cos_cutoff; info->nb_channels = o->nch;
    for (int i = 0; i < o->nch * 9; ++i) info->sky_params[i] = o->sky_params[i];
    for (int i = 0; i < o->nch; ++i) info->sky_radiance[i] = o->sky_rad[i];
    for (int i = 0; i < 100; ++i) info->gaussians[i] = o->gaussians[i];
    for (int i = 0; i < 20; ++i) info->gauss_cdf[i] = o->gauss_cdf[i];
    info->gauss_sum = o->gauss_sum;
    info->spec_size = o->spec_size;
    for (int i = 0; i < o->spec_size; ++i) info->spec_pdf[i] = o->spec_pdf[i];
    for (int i = 0; i + 1 < o->spec_size; ++i) info->spec_cdf[i] = o->spec_cdf[i];
    info->spec_integral = o->spec_integral;
}

void N_(oracle_override_w_sky)(O_T *o, double w_sky) { o->w_sky = (R)w_sky; }

/* The reference holds its staged tables in fp32 (array_from_file<Float64, Float>,
   sunsky.cpp:182-195; compute_radiance_params / compute_sun_params in Float).  These two hooks
   give the R evaluation of fp32 tables -- in the f64 instantiation, the exact value of the
   fp32-staged algorithm -- so a kernel's error splits into table rounding (o64 against this)
   and its own arithmetic (the kernel against this):
   round: every staged radiance table (sky coefficients, sky radiance, turbidity-lerped sun
          table, limb darkening) rounded to fp32 in place;
   adopt: the tables replaced by another implementation's fp32 staging (counts must match),
          and with them its fp32 local sun direction and disc cutoff: a fp64 renormalisation
          of the fp32 direction moves it by ~1e-8, which at the limb (d cos psi / d gamma
          unbounded) moves a disc lane by up to ~5e-5 -- the input, not the arithmetic.
   Both switch render_sun to the fp32 segment decision. */
void N_(oracle_round_staged_tables)(O_T *o) {
    const int nsun = o->spectral ? 45 * 11 * 4 : 45 * 3 * 4 * 6;
    for (int i = 0; i < o->nch * 9; ++i) o->sky_params[i] = (R)(float)o->sky_params[i];
    for (int i = 0; i < o->nch; ++i) o->sky_rad[i] = (R)(float)o->sky_rad[i];
    for (int i = 0; i < nsun; ++i) o->sun_rad[i] = (R)(float)o->sun_rad[i];
    for (int i = 0; i < 11 * 6; ++i) o->sun_ld[i] = (R)(float)o->sun_ld[i];
    o->seg_f32 = 1;
}

int N_(oracle_adopt_tables)(O_T *o, const float *sky_params, size_t n_sky, const float *sky_rad, size_t n_rad,
                            const float *sun_rad, size_t n_sun, const float *sun_ld, size_t n_ld,
                            const float *sun_local, float cos_cutoff, float area_ratio) {
    const size_t nsun = o->spectral ? 45 * 11 * 4 : 45 * 3 * 4 * 6;
    if (n_sky != (size_t)o->nch * 9 || n_rad != (size_t)o->nch || n_sun != nsun || n_ld != 11 * 6) {
        set_error("oracle: adopt_tables sizes %zu %zu %zu %zu do not match the emitter", n_sky, n_rad, n_sun, n_ld);
        return 1;
    }
    for (size_t i = 0; i < n_sky; ++i) o->sky_params[i] = (R)sky_params[i];
    for (size_t i = 0; i < n_rad; ++i) o->sky_rad[i] = (R)sky_rad[i];
    for (size_t i = 0; i < n_sun; ++i) o->sun_rad[i] = (R)sun_rad[i];
    for (size_t i = 0; i < n_ld; ++i) o->sun_ld[i] = (R)sun_ld[i];
    if (sun_local) {
        V3 n = { (R)sun_local[0], (R)sun_local[1], (R)sun_local[2] };
        o->sun_dir_local = n;
        o->frame.n = n;
        N_(coordinate_system)(o->frame.n, &o->frame.s, &o->frame.t);
        o->cos_cutoff = (R)cos_cutoff;
    }
    /* get_area_ratio (sunsky.h:99-101) in fp32 cancels in 1 - cos(half aperture): away from
       the default aperture (where the ratio is exactly 1) the fp32 staged ratio differs from
       the fp64 one by up to ~2e-3, a scale of the whole disc term that the kernels take as
       given */
    if (area_ratio >= 0) o->area_ratio = (R)area_ratio;
    o->seg_f32 = 1;
    return 0;
}

/* The nodes of m_spectral_distr come out of the 200x200 quadrature (sunsky.cpp:870-885),
   staged independently on both sides; adopting the other side's nodes isolates the
   sampling (ContinuousDistribution::sample_pdf, distr_1d.h:468-499).  The CDF is rebuilt
   here by the oracle's own restatement of compute_cdf, so the adopting side's CDF build
   stays under test. */
int N_(oracle_override_spectral_distr)(O_T *o, const double *pdf, int size) {
    if (size < 2 || size > 10) { set_error("oracle: spectral distribution size %d not in [2, 10]", size); return 1; }
    for (int i = 0; i < size; ++i)
        if (!(pdf[i] >= 0) || !isfinite(pdf[i])) { set_error("oracle: spectral pdf[%d] = %g", i, pdf[i]); return 1; }
    o->spec_size = size;
    for (int i = 0; i < size; ++i) o->spec_pdf[i] = (R)pdf[i];
    N_(build_spectral_distr)(o);
    return 0;
}

size_t N_(oracle_sun_table)(const O_T *o, R *out, size_t cap) {
    size_t n = o->spectral ? 45 * 11 * 4 : 45 * 3 * 4 * 6;
    for (size_t i = 0; i < n && i < cap; ++i) out[i] = o->sun_rad[i];
    return n;
}

void N_(oracle_eval)(const O_T *o, const float *wx, const float *wy, const float *wz,
                     const float *lambda, int n_lambda, size_t n, R *out) {
    long long nn = (long long)n;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < nn; ++i) {
        V3 wi = { -(R)wx[i], -(R)wy[i], -(R)wz[i] };
        V3 wo = N_(xform_vec)(o->to_local, wi);
        if (!o->spectral) {
            R r[3];
            N_(eval_local)(o, wo, 0, r);
            out[i] = r[0]; out[n + i] = r[1]; out[2 * n + i] = r[2];
        } else {
            for (int k = 0; k < n_lambda; ++k) {
                R r[3]; /* eval_local's RGB-sized buffer (one entry used here) */
                N_(eval_local)(o, wo, (R)lambda[(size_t)k * n + i], r);
                out[(size_t)k * n + i] = r[0];
            }
        }
    }
}

/* sample_direction, sunsky.cpp:399-441 */
void N_(oracle_sample_direction)(const O_T *o, const float *ux, const float *uy,
                                 const float *px, const float *py, const float *pz,
                                 const float *lambda, int n_lambda, size_t n,
                                 R *dx, R *dy, R *dz, R *pdf, R *dist, R *weight) {
    long long nn = (long long)n;
    int nw = o->spectral ? n_lambda : 3;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < nn; ++i) {
        R sx = ux[i], sy = uy[i];
        int pick_sky = sx < o->w_sky;
        V3 sd = pick_sky ? N_(sample_sky)(o, sx / o->w_sky, sy)
                         : N_(sample_sun)(o, (sx - o->w_sky) / (1 - o->w_sky), sy);
        int active = sd.z >= 0;
        V3 itp = { px ? px[i] : 0, py ? py[i] : 0, pz ? pz[i] : 0 };
        V3 rel = { itp.x - o->bs_center[0], itp.y - o->bs_center[1], itp.z - o->bs_center[2] };
        R nrm = N_(norm)(rel);
        R radius = o->bs_radius > nrm ? o->bs_radius : nrm;
        V3 d = N_(xform_vec)(o->to_world, sd);
        R skyp, sunp;
        N_(compute_pdfs)(o, sd, pick_sky, active, &skyp, &sunp);
        R pd = N_(lerp)(sunp, skyp, o->w_sky);
        dx[i] = d.x; dy[i] = d.y; dz[i] = d.z;
        pdf[i] = pd;
        if (dist) dist[i] = 2 * radius;
        /* eval(si{wi = -d}) / pdf, masked by active, zeroed if non-finite */
        V3 wo = N_(xform_vec)(o->to_local, d);
        R e[16]; /* up to 16 wavelengths per sample (kMaxLambdaPerRay), one entry each */
        if (!o->spectral)
            N_(eval_local)(o, wo, 0, e);
        else
            for (int k = 0; k < nw; ++k) N_(eval_local)(o, wo, (R)lambda[(size_t)k * n + i], e + k);
        for (int k = 0; k < nw; ++k) {
            R v = (active ? e[k] : (R)0) / pd;
            if (!isfinite(v)) v = 0;
            weight[(size_t)k * n + i] = v;
        }
    }
}

/* pdf_direction, sunsky.cpp:443-451 */
void N_(oracle_pdf_direction)(const O_T *o, const float *dx, const float *dy, const float *dz,
                              size_t n, R *pdf) {
    long long nn = (long long)n;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < nn; ++i) {
        V3 d = { dx[i], dy[i], dz[i] };
        V3 l = N_(xform_vec)(o->to_local, d);
        R skyp, sunp;
        N_(compute_pdfs)(o, l, 1, 1, &skyp, &sunp);
        pdf[i] = N_(lerp)(sunp, skyp, o->w_sky);
    }
}

/* sample_ray, sunsky.cpp:354-397 + sample_wavelengths :463-480 */
void N_(oracle_sample_ray)(const O_T *o, const float *wavelength_sample,
                           const float *s2x, const float *s2y, const float *s3x,
                           const float *s3y, size_t n, R *ox, R *oy, R *oz, R *dxo, R *dyo,
                           R *dzo, R *lambda_out, R *weight) {
    long long nn = (long long)n;
    int nw = o->spectral ? 4 : 3;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < nn; ++i) {
        R offx, offy;
        N_(disk_concentric)(s2x[i], s2y[i], &offx, &offy);
        R sx = s3x[i], sy = s3y[i];
        int pick_sky = sx < o->w_sky;
        V3 d = pick_sky ? N_(sample_sky)(o, sx / o->w_sky, sy)
                        : N_(sample_sun)(o, (sx - o->w_sky) / (1 - o->w_sky), sy);
        V3 nd = { -d.x, -d.y, -d.z };
        V3 dw = N_(xform_vec)(o->to_world, nd);
        int active = d.z >= 0;
        R skyp, sunp;
        N_(compute_pdfs)(o, d, pick_sky, active, &skyp, &sunp);
        R pd = N_(lerp)(sunp, skyp, o->w_sky);
        pd *= ((R)0.31830988618379067154) * ((R)1 / (o->bs_radius * o->bs_radius));
        active = active && pd > 0;
        /* eval(si{wi = d_world}): local_wo = M^-1 (-d_world) */
        V3 mdw = { -dw.x, -dw.y, -dw.z };
        V3 wo = N_(xform_vec)(o->to_local, mdw);
        R w[4];
        if (!o->spectral) {
            R e[3];
            N_(eval_local)(o, wo, 0, e);
            for (int c = 0; c < 3; ++c) w[c] = active ? e[c] : (R)0;
            if (lambda_out) for (int k = 0; k < 4; ++k) lambda_out[(size_t)k * n + i] = 0;
        } else {
            R ws = wavelength_sample[i];
            for (int k = 0; k < 4; ++k) {
                R s = ws + (R)k / (R)4;   /* sample_shifted, math.h:408-431 */
                if (s > 1) s -= 1;
                R lpdf;
                R lam = N_(cont_sample_pdf)(o, s, &lpdf);
                R e[3];
                N_(eval_local)(o, wo, lam, e);
                w[k] = (active ? e[0] : (R)0) / lpdf;
                lambda_out[(size_t)k * n + i] = lam;
            }
        }
        /* Frame(d_world).to_world(offset, 0) */
        FRAME fr;
        fr.n = dw;
        N_(coordinate_system)(dw, &fr.s, &fr.t);
        V3 off = { offx, offy, 0 };
        V3 po = N_(to_world)(&fr, off);
        ox[i] = o->bs_center[0] + (po.x - dw.x) * o->bs_radius;
        oy[i] = o->bs_center[1] + (po.y - dw.y) * o->bs_radius;
        oz[i] = o->bs_center[2] + (po.z - dw.z) * o->bs_radius;
        dxo[i] = dw.x; dyo[i] = dw.y; dzo[i] = dw.z;
        for (int k = 0; k < nw; ++k) {
            R v = w[k] / pd;
            if (!isfinite(v)) v = 0;
            weight[(size_t)k * n + i] = v;
        }
    }
}

/* sample_wavelengths, sunsky.cpp:463-480: spectral variants draw 4 shifted samples
   (math::sample_shifted, math.h:408-431) from the lambda distribution
   (ContinuousDistribution::sample_pdf, distr_1d.h:468-499) and weight eval(si) by
   1/pdf -- no non-finite zeroing there, unlike sample_direction.  RGB variants return
   lambda = 0 and eval(si). */
void N_(oracle_sample_wavelengths)(const O_T *o, const float *wx, const float *wy, const float *wz,
                                   const float *sample, size_t n, R *lambda_out, R *weight) {
    long long nn = (long long)n;
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < nn; ++i) {
        V3 wi = { -(R)wx[i], -(R)wy[i], -(R)wz[i] };
        V3 wo = N_(xform_vec)(o->to_local, wi);
        if (!o->spectral) {
            R r[3];
            N_(eval_local)(o, wo, 0, r);
            for (int c = 0; c < 3; ++c) weight[(size_t)c * n + i] = r[c];
            for (int k = 0; k < 4; ++k) lambda_out[(size_t)k * n + i] = 0;
            continue;
        }
        for (int k = 0; k < 4; ++k) {
            R s = (R)sample[i] + (R)k / (R)4;
            if (s > 1) s -= 1;
            R lpdf, e[3];
            R lam = N_(cont_sample_pdf)(o, s, &lpdf);
            N_(eval_local)(o, wo, lam, e);
            lambda_out[(size_t)k * n + i] = lam;
            weight[(size_t)k * n + i] = e[0] / lpdf;
        }
    }
}

/* arhosekskymodel_solar_radiance_internal2 (ArHosekSkyModel.c:686-784),
   restated on the reordered sun_spec_rad table (sunsky.h:777-809) and LD table.
   Always fp64-style control flow; R precision arithmetic. */
R N_(oracle_hw_sun_radiance)(const O_T *o, R turbidity, R wavelength, R elevation, R gamma) {
    if (!(wavelength >= 320 && wavelength <= 720 && turbidity >= 1 && turbidity <= 10)) return 0;
    int turb_low = (int)turbidity - 1;
    R turb_frac = turbidity - (R)(turb_low + 1);
    if (turb_low == 9) { turb_low = 8; turb_frac = 1; }
    int wl_low = (int)((wavelength - 320) / 40);
    R wl_frac = F(fmod)(wavelength, (R)40) / 40;
    if (wl_low == 10) { wl_low = 9; wl_frac = 1; }
    R rad[2][2];
    for (int t = 0; t < 2; ++t)
        for (int l = 0; l < 2; ++l) {
            int pos = (int)(F(pow)(2 * elevation / PI_, (R)1 / 3) * 45);
            if (pos > 44) pos = 44;
            R break_x = F(pow)((R)pos / 45, (R)3) * (PI_ * (R)0.5);
            const R *c = o->sun_rad_ds + (((size_t)(turb_low + t) * 45 + pos) * 11 + (wl_low + l)) * 4;
            R x = elevation - break_x, xe = 1, res = 0;
            for (int i = 0; i < 4; ++i) { res += xe * c[i]; xe *= x; }
            rad[t][l] = res;
        }
    R direct = (1 - turb_frac) * ((1 - wl_frac) * rad[0][0] + wl_frac * rad[0][1]) +
               turb_frac * ((1 - wl_frac) * rad[1][0] + wl_frac * rad[1][1]);
    R ld[6];
    for (int i = 0; i < 6; ++i)
        ld[i] = (1 - wl_frac) * o->sun_ld[wl_low * 6 + i] + wl_frac * o->sun_ld[(wl_low + 1) * 6 + i];
    R s = F(sin)((R)(0.5358 / 2.0 * (3.14159265358979323846 / 180.0)));
    R ar2 = 1 / (s * s), sg = F(sin)(gamma);
    R sc2 = (R)1 - ar2 * sg * sg;
    if (sc2 < 0) sc2 = 0;
    R sc = F(sqrt)(sc2);
    R dark = ld[0] + ld[1] * sc + ld[2] * F(pow)(sc, (R)2) + ld[3] * F(pow)(sc, (R)3) +
             ld[4] * F(pow)(sc, (R)4) + ld[5] * F(pow)(sc, (R)5);
    return direct * dark;
}

#undef V3
#undef FRAME
#undef PI_
#undef O_T
#undef N_
