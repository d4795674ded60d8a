#include "sunsky_kernels.hip"
// math_probe.hip -- probe kernels over the FAST device math of sunsky_kernels.hip
// (tests/math_probe.py, tests/test_gpu_device_math.py, tools/device_math_measure.py).  The
// product's translation unit is included above as it stands (its fp contract(on) pragma and
// every primitive by name, nothing copied); tests/cpp/Makefile builds this file with the
// product's HIPFLAGS into tests/cpp/build/math_probe.hsaco.  Not part of the product.
//
// Two kernel shapes per primitive:
//  * sweep: math_probe_sweep_<name>(first, count, rows, out, aux, aux_n) visits the
//    arguments first .. first + count - 1 grid-stride (a one-argument primitive: the fp32
//    bit pattern; a two-argument one: an index its functor decodes, mirrored by
//    tests/math_probe.py), computes the fp32 result and an fp64 reference with the
//    device's double libm in the same thread, and writes ONE row of 6 64-bit words per
//    block (rows must equal gridDim.x): max error in fp32 ulps at the reference (floor: the
//    smallest normal) as a double, its argument, max absolute error as a double, its
//    argument, the count of arguments with a non-finite result or reference or a failed
//    range / sign check, the count visited.  Plain vector stores, no atomics.
//  * values: math_probe_values(fn, x, y, out0, out1, n) returns the fp32 results for a
//    host-supplied list.
namespace math_probe {

typedef unsigned long long u64;
constexpr u64 kNone = ~0ull;             // "no argument": the row's maximum is 0
constexpr u64 kUnitFloats = 0x3f800001;  // the floats of [0, 1]
constexpr u64 kBelowOne = 0x3f800000;    // the floats of [0, 1)

struct Err {
    double ulp, abs;
    unsigned bad;
};

__device__ __forceinline__ float f_of(u64 bits) { return __uint_as_float((unsigned)bits); }

// |got - ref| in ulps of fp32 at ref (ulp = 2^(max(floor(log2 |ref|), -126) - 23)) and absolute
__device__ __forceinline__ Err err_of(float got, double ref) {
    Err e{0.0, 0.0, 0u};
    if (!__builtin_isfinite(got) || !__builtin_isfinite(ref)) {
        e.bad = 1u;
        return e;
    }
    int ex = 0;
    (void)frexp(ref, &ex);   // |ref| in [2^(ex - 1), 2^ex)
    ex = ref == 0.0 ? -126 : (ex - 1 < -126 ? -126 : ex - 1);
    e.abs = fabs((double)got - ref);
    e.ulp = ldexp(e.abs, 23 - ex);
    return e;
}

// bit equality of the three quotients (NaN equals NaN): ulp = abs = 1 on a mismatch, counted in bad
__device__ __forceinline__ Err same_bits(float got, float q32, float q64) {
    const bool nan3 = got != got && q32 != q32 && q64 != q64;
    const bool eq = __float_as_uint(got) == __float_as_uint(q32) && __float_as_uint(q32) == __float_as_uint(q64);
    const double m = (nan3 || eq) ? 0.0 : 1.0;
    return Err{m, m, (nan3 || eq) ? 0u : 1u};
}

struct Rcp { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(fast_rcp(x), 1.0 / (double)x); } };
struct Rsq { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(fast_rsq(x), 1.0 / sqrt((double)x)); } };
struct Sqrt { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(fast_sqrt(x), sqrt((double)x)); } };
struct Exp2 { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(fast_exp2(x), exp2((double)x)); } };
struct Log2 { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(__builtin_amdgcn_logf(x), log2((double)x)); } };
struct Asin { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(asin_half_chord(x), asin((double)x)); } };
struct Atan { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(atan_unit(x), atan((double)x)); } };

// elevation_fast against asin z; bad: a result outside [0, pi/2] (the fp32 constant)
struct Elevation {
    static __device__ Err at(u64 i, const float*, u64) {
        const float z = f_of(i), got = elevation_fast(z);
        Err e = err_of(got, asin((double)z));
        if (!(got >= 0.f && got <= kHalfPi)) e.bad = 1u;
        return e;
    }
};

template <bool COS>
struct SinCos {
    static __device__ Err at(u64 i, const float*, u64) {
        const float x = f_of(i);
        float s, c;
        sincos_fast(x, &s, &c);
        return COS ? err_of(c, cos((double)x)) : err_of(s, sin((double)x));
    }
};
// as SinCos, arguments whose reference is below 1e-3 in magnitude left out of the maxima
// (the qualifier of tools/fit_sincos.py's ulp figure)
template <bool COS>
struct SinCosBig {
    static __device__ Err at(u64 i, const float*, u64) {
        const float x = f_of(i);
        float s, c;
        sincos_fast(x, &s, &c);
        const double ref = COS ? cos((double)x) : sin((double)x);
        if (fabs(ref) <= 1e-3) return Err{0.0, 0.0, 0u};
        return err_of(COS ? c : s, ref);
    }
};
// sin(-x) = -sin(x), cos(-x) = cos(x) in bits: i is the pattern of x >= 0
struct SinCosParity {
    static __device__ Err at(u64 i, const float*, u64) {
        const float x = f_of(i);
        float s, c, sm, cm;
        sincos_fast(x, &s, &c);
        sincos_fast(-x, &sm, &cm);
        const double m = (__float_as_uint(sm) == (__float_as_uint(s) ^ 0x80000000u) &&
                          __float_as_uint(cm) == __float_as_uint(c)) ? 0.0 : 1.0;
        return Err{m, m, m == 0.0 ? 0u : 1u};
    }
};

struct ErfinvFast { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(erfinv_fast(x), erfinv((double)x)); } };
struct ErfinvRef { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(erfinvf_(x), erfinv((double)x)); } };
// the FAST form against the libm-log form
struct ErfinvPair { static __device__ Err at(u64 i, const float*, u64) { const float x = f_of(i); return err_of(erfinv_fast(x), (double)erfinvf_(x)); } };
// erfinv_fast(-x) = -erfinv_fast(x) in bits: i is the pattern of x >= 0
struct ErfinvOdd {
    static __device__ Err at(u64 i, const float*, u64) {
        const float x = f_of(i);
        const double m = __float_as_uint(erfinv_fast(-x)) == (__float_as_uint(erfinv_fast(x)) ^ 0x80000000u) ? 0.0 : 1.0;
        return Err{m, m, m == 0.0 ? 0u : 1u};
    }
};

// wavelength_node against the device's IEEE quotient and the fp64 quotient rounded once
struct Wavelength {
    static __device__ Err at(u64 i, const float*, u64) {
        const float lambda = f_of(i), a = lambda - kWavelength0;
        return same_bits(wavelength_node(lambda), a / kWavelengthStep, (float)((double)a / (double)kWavelengthStep));
    }
};

// div_by_rcp(a, b, RN(1 / b)): index = j * 0x3f800000 + bits(a), a every float of [0, 1),
// b = aux[j]
struct DivByRcp {
    static __device__ Err at(u64 i, const float* aux, u64 aux_n) {
        const u64 j = i / kBelowOne;
        if (j >= aux_n) return Err{0.0, 0.0, 1u};
        const float a = f_of(i % kBelowOne), b = aux[j], rb = 1.f / b;
        return same_bits(div_by_rcp(a, b, rb), a / b, (float)((double)a / (double)b));
    }
};

// bad: |result| above the fp32 pi or a sign that is not y's
__device__ __forceinline__ Err atan2_err(float y, float x) {
    const float got = atan2_fast(y, x);
    Err e = err_of(got, atan2((double)y, (double)x));
    if (!(fabsf(got) <= kPi) || signbit(got) != signbit(y)) e.bad = 1u;
    return e;
}
// (1, t), t every float of [0, 1], in 8 octants: index = oct * 0x3f800001 + bits(t);
// oct bit 0 swaps the components, bit 1 negates x, bit 2 negates y
struct Atan2Octant {
    static __device__ Err at(u64 i, const float*, u64) {
        const unsigned oct = (unsigned)(i / kUnitFloats);
        float x = 1.f, y = f_of(i % kUnitFloats);
        if (oct > 7u) return Err{0.0, 0.0, 1u};
        if (oct & 1u) { const float t = x; x = y; y = t; }
        if (oct & 2u) x = -x;
        if (oct & 4u) y = -y;
        return atan2_err(y, x);
    }
};
// the unit circle at 2^24 angles scaled by 2^(-4 s): index = s * 2^24 + k, angle 2 pi k / 2^24
constexpr u64 kCirclePoints = 16ull << 24;
__device__ __forceinline__ void circle_point(u64 i, float* y, float* x) {
    const int s = (int)(i >> 24);
    double sn, cs;
    sincos(6.283185307179586476925 * (double)(i & 0xffffffull) * 0x1p-24, &sn, &cs);
    *y = (float)ldexp(sn, -4 * s);
    *x = (float)ldexp(cs, -4 * s);
}
struct Atan2Circle {
    static __device__ Err at(u64 i, const float*, u64) {
        if (i >= kCirclePoints) return Err{0.0, 0.0, 1u};
        float y, x;
        circle_point(i, &y, &x);
        return atan2_err(y, x);
    }
};

// theta_upper_fast against the fp64 chord form 2 asin(|v - e_z| / 2) of the same fp32 vector.
// index < 2^24: z = (j + 1/2) / 4096, azimuth 2 pi (k + 1/2) / 4096 with j = index >> 12,
// k = index & 4095; then 2^20 points of rings at polar angle 1e-3 (j + 1/2) / 256 (j < 256), then
// 2^20 at pi/2 - 1e-3 (j + 1/2) / 256
constexpr u64 kThetaPoints = (1ull << 24) + (2ull << 20);
__device__ __forceinline__ float3_ theta_vector(u64 i) {
    const double phi = 6.283185307179586476925 * ((double)(i & 4095ull) + 0.5) / 4096.0;
    double z, st;
    if (i < (1ull << 24)) {
        z = ((double)(i >> 12) + 0.5) / 4096.0;
        st = sqrt(1.0 - z * z);
    } else {
        const u64 r = i - (1ull << 24);
        double th = 1e-3 * ((double)((r >> 12) & 255ull) + 0.5) / 256.0;
        if (r >> 20) th = 1.5707963267948966 - th;
        sincos(th, &st, &z);
    }
    return mk3((float)(st * cos(phi)), (float)(st * sin(phi)), (float)z);
}
struct ThetaUpper {
    static __device__ Err at(u64 i, const float*, u64) {
        if (i >= kThetaPoints) return Err{0.0, 0.0, 1u};
        const float3_ v = theta_vector(i);
        const double dz = (double)v.z - 1.0;
        const double ref = 2.0 * asin(0.5 * sqrt((double)v.x * v.x + (double)v.y * v.y + dz * dz));
        return err_of(theta_upper_fast(v), ref);
    }
};

// The sun directions of the dir_terms sweep: elevation 0.1, 30 and 89.5 degrees in the x-z plane
__device__ __forceinline__ void sun_frame(unsigned s, double* ce, double* se) {
    const double el = (s == 0 ? 0.1 : s == 1 ? 30.0 : 89.5) * 0.017453292519943295;
    sincos(el, se, ce);
}
// dir_terms<true>'s gamma and cos gamma.  index = s * 2^21 + r, s the sun (3).  r < 2^20: the
// hemisphere grid z = (j + 1/2) / 1024, azimuth 2 pi (k + 1/2) / 1024 (j = r >> 10, k = r & 1023).
// Then 2^20 points on 256 rings of 4096 azimuths around the sun, ring j at angle
//   j < 128:  1e-6 * 4650^(j / 127)             (1e-6 to the disc edge, 4.65e-3)
//   j < 192:  pi/2 + (j - 160) * 2^-25          (d changes sign across these)
//   else:     pi - 1e-6 * 1000^((j - 192) / 63)
constexpr u64 kDirPoints = 3ull << 21;
__device__ __forceinline__ void dir_inputs(u64 i, float3_* sn, float3_* wo) {
    const unsigned s = (unsigned)(i >> 21);
    const u64 r = i & ((1ull << 21) - 1);
    double ce, se;
    sun_frame(s, &ce, &se);
    *sn = mk3((float)ce, 0.f, (float)se);
    if (r < (1ull << 20)) {
        const double z = ((double)(r >> 10) + 0.5) / 1024.0, st = sqrt(1.0 - z * z);
        const double phi = 6.283185307179586476925 * ((double)(r & 1023ull) + 0.5) / 1024.0;
        *wo = mk3((float)(st * cos(phi)), (float)(st * sin(phi)), (float)z);
        return;
    }
    const int j = (int)((r >> 12) & 255ull);
    const double phi = 6.283185307179586476925 * ((double)(r & 4095ull) + 0.5) / 4096.0;
    double g;
    if (j < 128) g = 1e-6 * pow(4650.0, (double)j / 127.0);
    else if (j < 192) g = 1.5707963267948966 + (double)(j - 160) * 0x1p-25;
    else g = 3.141592653589793 - 1e-6 * pow(1000.0, (double)(j - 192) / 63.0);
    double sg, cg, sp, cp;
    sincos(g, &sg, &cg);
    sincos(phi, &sp, &cp);
    // sn cos g + (e1 cos phi + e2 sin phi) sin g with e1 = (0, 1, 0), e2 = (-se, 0, ce)
    *wo = mk3((float)(ce * cg - se * sp * sg), (float)(cp * sg), (float)(se * cg + ce * sp * sg));
}
// fp64 of the same form on the same fp32 vectors: 2 asin(|wo -/+ sn| / 2) (pi minus it on the
// far side), the side taken from the sign of the product's own fp32 dot3
__device__ __forceinline__ void dir_reference(float3_ sn, float3_ wo, double* gamma, double* cosg) {
    const bool far = signbit(dot3(sn, wo));
    const double sgn = far ? -1.0 : 1.0;
    const double vx = (double)wo.x - sgn * sn.x, vy = (double)wo.y - sgn * sn.y, vz = (double)wo.z - sgn * sn.z;
    const double h2 = 0.25 * (vx * vx + vy * vy + vz * vz);
    const double t = 2.0 * asin(sqrt(h2));
    *gamma = far ? 3.14159265358979323846 - t : t;
    *cosg = far ? -(1.0 - 2.0 * h2) : 1.0 - 2.0 * h2;
}
template <bool COS>
struct DirAngle {
    static __device__ Err at(u64 i, const float*, u64) {
        if (i >= kDirPoints) return Err{0.0, 0.0, 1u};
        float3_ sn, wo;
        dir_inputs(i, &sn, &wo);
        SunskyKArgs K;
        K.sun_n[0] = sn.x; K.sun_n[1] = sn.y; K.sun_n[2] = sn.z;
        K.cos_cutoff = 0.99998919f;
        const DirTerms t = dir_terms<true>(K, wo, true);
        double g, c;
        dir_reference(sn, wo, &g, &c);
        return COS ? err_of(t.cg, c) : err_of(t.gamma, g);
    }
};

// disk_concentric_dev<true> on the grid (sx, sy) = (k, j) / 4096 (index = j * 4096 + k), which
// holds the centre, the axes and the diagonals |x| = |y| of x = 2 sx - 1, y = 2 sy - 1, against
// the fp64 map.  ulp: the larger component error in units of 2^-24; bad: px^2 + py^2 above
// 1 + kDiskSlack in fp64 (a unit r times a cosine and a sine rounded to fp32 is not within the disk)
__device__ __forceinline__ void disk_reference(double sx, double sy, double* px, double* py) {
    const double x = 2.0 * sx - 1.0, y = 2.0 * sy - 1.0;
    const bool q13 = fabs(x) < fabs(y);
    const double r = q13 ? y : x, rp = q13 ? x : y;
    double phi = (x == 0.0 && y == 0.0) ? 0.0 : 0.78539816339744830962 * rp / r;
    if (q13) phi = 1.5707963267948966192 - phi;
    if (x == 0.0 && y == 0.0) phi = 0.0;
    double s, c;
    sincos(phi, &s, &c);
    *px = r * c;
    *py = r * s;
}
constexpr u64 kGridPoints = 1ull << 24;
constexpr double kDiskSlack = 4.3e-7;   // tests/math_probe.py DISK_SLACK
struct Disk {
    static __device__ Err at(u64 i, const float*, u64) {
        if (i >= kGridPoints) return Err{0.0, 0.0, 1u};
        const float sx = (float)(i & 4095ull) * 0x1p-12f, sy = (float)(i >> 12) * 0x1p-12f;
        float px, py;
        disk_concentric_dev<true>(sx, sy, &px, &py);
        double rx, ry;
        disk_reference((double)sx, (double)sy, &rx, &ry);
        Err e{0.0, 0.0, 0u};
        if (!__builtin_isfinite(px) || !__builtin_isfinite(py)) { e.bad = 1u; return e; }
        e.abs = fmax(fabs((double)px - rx), fabs((double)py - ry));
        e.ulp = e.abs * 0x1p24;
        if ((double)px * px + (double)py * py > 1.0 + kDiskSlack) e.bad = 1u;
        return e;
    }
};
// uniform_cone_dev<true> on the same grid at aperture s = index >> 24: the default sun half
// aperture (0.2665 degrees), 5 and 30 degrees, against the fp64 map with the same fp32
// cos_cutoff.  ulp: the largest component error in units of 2^-24; bad: z < cos_cutoff
__device__ __forceinline__ float cone_cutoff(unsigned s) {
    return (float)cos((s == 0 ? 0.2665 : s == 1 ? 5.0 : 30.0) * 0.017453292519943295);
}
constexpr u64 kConePoints = 3ull << 24;
struct Cone {
    static __device__ Err at(u64 i, const float*, u64) {
        if (i >= kConePoints) return Err{0.0, 0.0, 1u};
        const float cc = cone_cutoff((unsigned)(i >> 24));
        const float sx = (float)(i & 4095ull) * 0x1p-12f, sy = (float)((i >> 12) & 4095ull) * 0x1p-12f;
        const float3_ v = uniform_cone_dev<true>(sx, sy, cc);
        double rx, ry;
        disk_reference((double)sx, (double)sy, &rx, &ry);
        const double omc = 1.0 - (double)cc, pn = rx * rx + ry * ry;
        const double sc = sqrt(fmax(omc * (2.0 - omc * pn), 0.0));
        Err e{0.0, 0.0, 0u};
        if (!__builtin_isfinite(v.x) || !__builtin_isfinite(v.y) || !__builtin_isfinite(v.z)) { e.bad = 1u; return e; }
        e.abs = fmax(fmax(fabs((double)v.x - rx * sc), fabs((double)v.y - ry * sc)),
                     fabs((double)v.z - ((double)cc + omc * (1.0 - pn))));
        e.ulp = e.abs * 0x1p24;
        if (v.z < cc) e.bad = 1u;
        return e;
    }
};

template <class F>
__device__ __forceinline__ void sweep(u64 first, u64 count, u64 rows, u64* out, const float* aux, u64 aux_n) {
    __shared__ double s_ulp[SS_BLOCK], s_abs[SS_BLOCK];
    __shared__ u64 s_ua[SS_BLOCK], s_aa[SS_BLOCK], s_bad[SS_BLOCK], s_n[SS_BLOCK];
    if (rows != gridDim.x || blockDim.x != SS_BLOCK) return;   // out holds one row per block
    double mu = 0.0, ma = 0.0;
    u64 ua = kNone, aa = kNone, bad = 0, n = 0;
    const u64 stride = (u64)gridDim.x * SS_BLOCK;
    for (u64 i = (u64)blockIdx.x * SS_BLOCK + threadIdx.x; i < count; i += stride) {
        const Err e = F::at(first + i, aux, aux_n);
        if (e.ulp > mu) { mu = e.ulp; ua = first + i; }
        if (e.abs > ma) { ma = e.abs; aa = first + i; }
        bad += e.bad;
        ++n;
    }
    const unsigned t = threadIdx.x;
    s_ulp[t] = mu; s_ua[t] = ua; s_abs[t] = ma; s_aa[t] = aa; s_bad[t] = bad; s_n[t] = n;
    __syncthreads();
    for (unsigned w = SS_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
            if (s_ulp[t + w] > s_ulp[t]) { s_ulp[t] = s_ulp[t + w]; s_ua[t] = s_ua[t + w]; }
            if (s_abs[t + w] > s_abs[t]) { s_abs[t] = s_abs[t + w]; s_aa[t] = s_aa[t + w]; }
            s_bad[t] += s_bad[t + w];
            s_n[t] += s_n[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        u64* row = out + 6 * (u64)blockIdx.x;
        row[0] = (u64)__double_as_longlong(s_ulp[0]);
        row[1] = s_ua[0];
        row[2] = (u64)__double_as_longlong(s_abs[0]);
        row[3] = s_aa[0];
        row[4] = s_bad[0];
        row[5] = s_n[0];
    }
}

}  // namespace math_probe

#define MATH_PROBE_SWEEP(name, F)                                                                        \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void math_probe_sweep_##name(                      \
        unsigned long long first, unsigned long long count, unsigned long long rows, unsigned long long* out, \
        const float* aux, unsigned long long aux_n) {                                                     \
        math_probe::sweep<math_probe::F>(first, count, rows, out, aux, aux_n);                            \
    }

MATH_PROBE_SWEEP(rcp, Rcp)
MATH_PROBE_SWEEP(rsq, Rsq)
MATH_PROBE_SWEEP(sqrt, Sqrt)
MATH_PROBE_SWEEP(exp2, Exp2)
MATH_PROBE_SWEEP(log2, Log2)
MATH_PROBE_SWEEP(asin_half_chord, Asin)
MATH_PROBE_SWEEP(elevation, Elevation)
MATH_PROBE_SWEEP(atan_unit, Atan)
MATH_PROBE_SWEEP(sin, SinCos<false>)
MATH_PROBE_SWEEP(cos, SinCos<true>)
MATH_PROBE_SWEEP(sin_big, SinCosBig<false>)
MATH_PROBE_SWEEP(cos_big, SinCosBig<true>)
MATH_PROBE_SWEEP(sincos_parity, SinCosParity)
MATH_PROBE_SWEEP(erfinv_fast, ErfinvFast)
MATH_PROBE_SWEEP(erfinv_ref, ErfinvRef)
MATH_PROBE_SWEEP(erfinv_pair, ErfinvPair)
MATH_PROBE_SWEEP(erfinv_odd, ErfinvOdd)
MATH_PROBE_SWEEP(wavelength_node, Wavelength)
MATH_PROBE_SWEEP(div_by_rcp, DivByRcp)
MATH_PROBE_SWEEP(atan2_octant, Atan2Octant)
MATH_PROBE_SWEEP(atan2_circle, Atan2Circle)
MATH_PROBE_SWEEP(theta_upper, ThetaUpper)
MATH_PROBE_SWEEP(dir_gamma, DirAngle<false>)
MATH_PROBE_SWEEP(dir_cos_gamma, DirAngle<true>)
MATH_PROBE_SWEEP(disk_concentric, Disk)
MATH_PROBE_SWEEP(uniform_cone, Cone)

// The fp32 results for a host-supplied list: out0[i] (and out1[i] where the primitive has a
// second output: the cosine, the libm-log erfinv, the IEEE quotient) for x[i] (and y[i]).  The fn
// numbers are the FN_* constants of tests/math_probe.py.
extern "C" __global__ __launch_bounds__(SS_BLOCK) void math_probe_values(int fn, const float* x, const float* y,
                                                                         float* out0, float* out1,
                                                                         unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * SS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float a = x[i], b = y[i];
    float r0 = 0.f, r1 = 0.f;
    switch (fn) {
    case 0: r0 = fast_rcp(a); break;
    case 1: r0 = fast_rsq(a); break;
    case 2: r0 = fast_sqrt(a); break;
    case 3: r0 = fast_exp2(a); break;
    case 4: r0 = __builtin_amdgcn_logf(a); break;
    case 5: r0 = asin_half_chord(a); break;
    case 6: r0 = elevation_fast(a); break;
    case 7: r0 = atan_unit(a); break;
    case 8: sincos_fast(a, &r0, &r1); break;
    case 9: r0 = erfinv_fast(a); r1 = erfinvf_(a); break;
    case 10: r0 = wavelength_node(a); r1 = (a - kWavelength0) / kWavelengthStep; break;
    case 11: r0 = div_by_rcp(a, b, 1.f / b); r1 = a / b; break;
    case 12: r0 = atan2_fast(a, b); break;   // (y, x)
    case 14: {   // dir_terms<true> at d = +0 (a > 0) or -0 (a < 0): sun at the zenith, wo = (a, b, 0 with a's sign)
        SunskyKArgs K;
        K.sun_n[0] = 0.f; K.sun_n[1] = 0.f; K.sun_n[2] = 1.f;
        K.cos_cutoff = 0.99998919f;
        const DirTerms t = dir_terms<true>(K, mk3(a, b, copysignf(0.f, a)), true);
        r0 = t.gamma;
        r1 = t.cg;
        break;
    }
    case 15: disk_concentric_dev<true>(a, b, &r0, &r1); break;
    case 16:
    case 17:
    case 18: {   // uniform_cone_dev<true> at aperture fn - 16: (x, y)
        const float3_ v = uniform_cone_dev<true>(a, b, math_probe::cone_cutoff((unsigned)(fn - 16)));
        r0 = v.x;
        r1 = v.y;
        break;
    }
    case 30:
    case 31:
    case 32: {   // uniform_cone_dev<true> at aperture fn - 30: (z, cos_cutoff)
        const float cc = math_probe::cone_cutoff((unsigned)(fn - 30));
        r0 = uniform_cone_dev<true>(a, b, cc).z;
        r1 = cc;
        break;
    }
    // the arguments the sweeps decode from an index (low word: x's bits, high word: y's)
    case 20:
    case 21:
    case 22: {
        const unsigned long long idx = ((unsigned long long)__float_as_uint(b) << 32) | __float_as_uint(a);
        if (fn == 20) {
            if (idx < math_probe::kCirclePoints) math_probe::circle_point(idx, &r0, &r1);   // (y, x)
        } else if (idx < math_probe::kThetaPoints) {
            const float3_ v = math_probe::theta_vector(idx);
            r0 = fn == 21 ? v.x : v.z;
            r1 = fn == 21 ? v.y : theta_upper_fast(v);
        }
        break;
    }
    case 23:
    case 24:
    case 25:
    case 26: {   // dir_terms sweep: (wo.x, wo.y), (wo.z, gamma), (sn.x, sn.z), (cos gamma, h)
        const unsigned long long idx = ((unsigned long long)__float_as_uint(b) << 32) | __float_as_uint(a);
        if (idx < math_probe::kDirPoints) {
            float3_ sn, wo;
            math_probe::dir_inputs(idx, &sn, &wo);
            SunskyKArgs K;
            K.sun_n[0] = sn.x; K.sun_n[1] = sn.y; K.sun_n[2] = sn.z;
            K.cos_cutoff = 0.99998919f;
            const DirTerms t = dir_terms<true>(K, wo, true);
            if (fn == 23) { r0 = wo.x; r1 = wo.y; }
            else if (fn == 24) { r0 = wo.z; r1 = t.gamma; }
            else if (fn == 25) { r0 = sn.x; r1 = sn.z; }
            else { r0 = t.cg; r1 = t.h; }
        }
        break;
    }
    default: break;
    }
    out0[i] = r0;
    out1[i] = r1;
}
