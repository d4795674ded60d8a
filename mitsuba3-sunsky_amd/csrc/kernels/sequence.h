// kernels/sequence.h -- frame sequences: the weighted sum of K frames' eval and bake, the sky-frame
// helpers the later sequence parts share (seq_sky_frame, seq_sky_sum), and the staging of the records.
// A part of sunsky_kernels.hip (one translation unit): included there, once, in order.

// ======================================================================
// Frame sequences (sunsky_sequence): out = sum_k w_k eval_k(wi) over K frames of one emitter
// that differ in sun direction and turbidity, in one launch.  A lane reads its direction once,
// forms the frame-independent terms once (wo, cos theta, r = 1 / (cos theta + 0.01),
// sqrt(cos theta)), then walks the frame records (SeqFrame, sunsky_kernel_args.h) with one
// address per wave: the records are read through the constant address space, so a frame's
// sun vector, weight and channel coefficients arrive by scalar loads into SGPRs, the next
// frame's issued before this frame's arithmetic.  Per frame the chord, gamma and cos gamma are
// dir_terms' arithmetic and the sky values sky_fast / sky_ref's, added as fma(w_k, v, acc) in
// frame order into fp32 accumulators; one non-temporal store per plane at the end.  The work
// is transcendental issue with next to no memory traffic.
// A lane inside frame k's disc takes a rare branch: the segment from the full threshold table,
// the disc coordinates by sun_disc64's arithmetic with the frame's sun vector, and the few
// sun-table entries it needs lerped on the spot from the raw dataset with the frame's
// turbidity scalars (sun_param: the bits of a single emitter's staged table), so a frame
// carries no sun table.  The branch reads the state and the record through opaque handles:
// none of its loads is hoisted into the frame loop.
// ======================================================================
typedef const __attribute__((address_space(4))) float* seq_cfloat_p;
typedef const __attribute__((address_space(4))) int* seq_cint_p;

constexpr int kSeqHeaderFloats = (int)(kSeqFrameHeader / 4);
constexpr int kSeqChanFloats = (int)((sizeof(FastChannel) + sizeof(SkyChannel)) / 4);

// record k of a sequence with nch channels, as floats in the constant address space
__device__ __forceinline__ seq_cfloat_p seq_record(const void* frames, int nch, int k) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    return (seq_cfloat_p)frames + (size_t)k * (size_t)(kSeqHeaderFloats + nch * kSeqChanFloats);
#pragma clang diagnostic pop
}

template <bool FAST>
__device__ __forceinline__ typename ChanSel<FAST>::T seq_chan(seq_cfloat_p rec, int nch, int c) {
    if constexpr (FAST) {
        seq_cfloat_p p = rec + kSeqHeaderFloats + c * 12;
        FastChannel f;
        f.A = p[0]; f.Bl2 = p[1]; f.El2 = p[2]; f.P = p[3]; f.Q = p[4];
        f.Cs = p[5]; f.Ds = p[6]; f.Fs = p[7]; f.Gs = p[8]; f.Hs = p[9];
        f.pad[0] = f.pad[1] = 0.f;
        return f;
    } else {
        seq_cfloat_p p = rec + kSeqHeaderFloats + nch * 12 + c * 16;
        SkyChannel s;
        s.A = p[0]; s.B = p[1]; s.C = p[2]; s.D = p[3]; s.E = p[4]; s.F = p[5]; s.G = p[6]; s.H = p[7]; s.I = p[8];
        s.P = p[9]; s.rad = p[10]; s.Bl2 = p[11]; s.El2 = p[12]; s.Q = p[13];
        s.pad[0] = s.pad[1] = 0.f;
        return s;
    }
}

// What the frame loop reads of one record: N channels starting at channel list c[]
template <bool FAST, int N>
struct SeqHot {
    float3_ sn;
    float w;
    typename ChanSel<FAST>::T ch[N];
};

template <bool FAST, int N>
__device__ __forceinline__ SeqHot<FAST, N> seq_load(const void* frames, int nch, int k, const int (&c)[N]) {
    seq_cfloat_p rec = seq_record(frames, nch, k);
    SeqHot<FAST, N> h;
    h.sn = mk3(rec[0], rec[1], rec[2]);
    h.w = rec[3];
#pragma unroll
    for (int i = 0; i < N; ++i) h.ch[i] = seq_chan<FAST>(rec, nch, c[i]);
    return h;
}

// The frame-independent part of dir_terms
struct SeqDir {
    float3_ wo;
    float r, sq;
    bool active;
};

template <bool FAST>
__device__ __forceinline__ SeqDir seq_dir(float3_ wo, bool mask) {
    SeqDir s;
    s.wo = wo;
    if (FAST) {
        s.r = fast_rcp(wo.z + 0.01f);
        s.sq = fast_sqrt(wo.z);   // NaN below the horizon: those lanes store 0
    } else {
        s.r = 1.f / (wo.z + 0.01f);
        s.sq = safe_sqrtf_(wo.z);
    }
    s.active = mask && (wo.z >= 0.f);
    return s;
}

// dir_terms' per-sun part for frame sun vector sn: the same statements, so a frame's terms are
// the bits its single emitter computes (the disc test included)
template <bool FAST>
__device__ __forceinline__ DirTerms seq_frame_terms(const SeqDir& s, float3_ sn, float cos_cutoff) {
    DirTerms t;
    const float3_ wo = s.wo;
    t.cos_theta = wo.z;
    float d = dot3(sn, wo);
    const float sg = signbit(d) ? -1.f : 1.f;
    float3_ v = mk3(fmaf(-sg, sn.x, wo.x), fmaf(-sg, sn.y, wo.y), fmaf(-sg, sn.z, wo.z));
    float h = 0.5f * (FAST ? fast_sqrt(dot3(v, v)) : sqrtf(dot3(v, v)));
    t.h = h;
    t.wx = wo.x;
    t.wy = wo.y;
    float temp = 2.f * (FAST ? asin_half_chord(h) : asinf(h));
    t.gamma = d >= 0.f ? temp : kPi - temp;
    if (FAST) {
        float c = fmaf(h * h, -2.f, 1.f);
        t.cg = d >= 0.f ? c : -c;
    } else {
        t.cg = cosf(t.gamma);
    }
    t.r = s.r;
    t.sq = s.sq;
    t.cg2 = t.cg * t.cg;
    t.u = 1.f + t.cg2;
    t.active = s.active;
    t.hit_sun = t.active && (d >= cos_cutoff);
    t.sun_pos = 0;
    t.sun_x = t.sun_cpsi = 0.f;
    return t;
}

// An index the compiler cannot see through (opaque_kargs' idiom for the record pointer)
__device__ __forceinline__ int seq_opaque(int k) {
    asm volatile("" : "+s"(k));
    return k;
}

// The turbidity lerp scalars of a record, for sun_param
__device__ __forceinline__ RadianceStage seq_sun_stage(seq_cfloat_p rec) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    seq_cint_p ri = (seq_cint_p)rec;
#pragma clang diagnostic pop
    RadianceStage rs;
    rs.x = 0.f;
    rs.t_rem = rec[4];
    rs.t_low = ri[5];
    rs.t_high = ri[6];
    rs.in_range = 1;
    return rs;
}

// sun_segment_index over the whole threshold table: it counts the thresholds a cos theta
// passes, so the index is the one an emitter's [sun_row_lo, sun_row_hi] window gives
__device__ __forceinline__ int seq_segment_index(const SunskyKArgs& K, float cos_theta) {
    int pos = 0;
#pragma unroll 1
    for (int j = 1; j < kNbSunSegments; ++j) pos += cos_theta >= K.sun_seg_z[j] ? 1 : 0;
    return pos;
}

// sun_disc64 with the frame's sun vector
__device__ __forceinline__ SunDisc64 seq_sun_disc64(const SunskyKArgs& K, float3_ sn, float wx, float wy,
                                                    float cos_theta) {
    SunDisc64 d;
    d.pos = seq_segment_index(K, cos_theta);
    const double frac = (double)d.pos * (1.0 / (double)kNbSunSegments);
    d.x = (double)elevation_fast(cos_theta) - 1.5707963267948966 * (frac * frac * frac);
    const double vx = (double)wx - (double)sn.x, vy = (double)wy - (double)sn.y, vz = (double)cos_theta - (double)sn.z;
    const double v2 = fma(vz, vz, fma(vy, vy, vx * vx));
    const double inv = (double)K.cpsi_inv_hi + (double)K.cpsi_inv_lo;
    d.cpsi = sqrt(fmax(fma(-inv, v2 * fma(-0.25, v2, 1.0), 1.0), 0.0));
    return d;
}

// The reference kernels' segment and x (sun_segment_ref)
__device__ __forceinline__ int seq_segment_ref(const SunskyKArgs& K, float cos_theta, float* x) {
    const int pos = seq_segment_index(K, cos_theta);
    const float elevation = kHalfPi - acosf(cos_theta);
    const float frac = (float)pos / (float)kNbSunSegments;
    *x = elevation - kHalfPi * (frac * frac * frac);
    return pos;
}

// The reference-precision disc term from its coordinates (segment pos, elevation xs within it,
// cos psi): what seq_disc_rgb<false> / seq_disc_spec<false> add for a direction, and what the
// irradiance flux rule evaluates at its nodes with cos psi given (sunsky_sequence_irradiance_flux)
__device__ __forceinline__ void seq_disc_rgb_at(const SunskyKArgs& Kf, const float* ds, int block, const RadianceStage& rs,
                                                int pos, float xs, float cpsi, float v[3]) {
    constexpr int per_c = kNbSunCtrlPts * kNbSunLdParams;
    const float conv = (float)kSpecToRgbSunConv;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        float s[per_c];
#pragma unroll
        for (int e = 0; e < per_c; ++e) s[e] = sun_param(ds, block, pos * (3 * per_c) + c * per_c + e, rs);
        v[c] += Kf.sun_scale * render_sun_rgb(s, 0, 0, xs, cpsi) * Kf.area_ratio * conv;
    }
}

// sun_spec_term<false>: render_sun_spec x sun_limb_darkening for the channel pair (lo, lo + 1, f)
__device__ __forceinline__ float seq_disc_spec_at(const SunskyKArgs& Kf, const float* ds, int block,
                                                  const RadianceStage& rs, int pos, float xs, float cpsi, int lo, float f,
                                                  float o) {
    const int hi = lo + 1;
    auto poly = [&](int c) {
        const int q = (pos * kNbWavelengths + c) * kNbSunCtrlPts;
        float res = 0.f;
#pragma unroll
        for (int e = 0; e < kNbSunCtrlPts; ++e) res += powif_(xs, e) * sun_param(ds, block, q + e, rs);
        return res;
    };
    const float sa = poly(lo);
    float sun = sa;
    if (f != 0.f) sun = lerpf_(sa, hi < kNbWavelengths ? poly(hi) : 0.f, f);
    const float ld = sun_limb_darkening(Kf.sun_ld, lo, hi, f, cpsi);
    return o + Kf.sun_scale * sun * ld * Kf.area_ratio;
}

// RGB disc term of frame k added to the lane's 3 sky values (the rare branch)
template <bool FAST>
__device__ __forceinline__ void seq_disc_rgb(const SunskyKArgs& K, const SeqArgs& A, int k, const DirTerms& t,
                                             float v[3]) {
    const SunskyKArgs& Kf = opaque_kargs(K);
    seq_cfloat_p rec = seq_record(A.frames, 3, seq_opaque(k));
    const RadianceStage rs = seq_sun_stage(rec);
    const float* ds = A.sun_rad_ds;
    const int block = A.sun_block;
    constexpr int per_c = kNbSunCtrlPts * kNbSunLdParams;
    if constexpr (FAST) {
        const SunDisc64 d = seq_sun_disc64(Kf, mk3(rec[0], rec[1], rec[2]), t.wx, t.wy, t.cos_theta);
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {   // add_sun_rgb64's Horner forms
            const int base = d.pos * (3 * per_c) + c * per_c;
            double res = 0.0;
#pragma unroll 1
            for (int q = kNbSunCtrlPts - 1; q >= 0; --q) {
                const int r = base + q * kNbSunLdParams;
                double inner = (double)sun_param(ds, block, r + kNbSunLdParams - 1, rs);
#pragma unroll
                for (int j = kNbSunLdParams - 2; j >= 0; --j) inner = fma(inner, d.cpsi, (double)sun_param(ds, block, r + j, rs));
                res = fma(res, d.x, inner);
            }
            v[c] = (float)fma((double)Kf.sun_mul, res, (double)v[c]);
        }
    } else {
        float xs;
        const int pos = seq_segment_ref(Kf, t.cos_theta, &xs);
        seq_disc_rgb_at(Kf, ds, block, rs, pos, xs, cos_psi(t.gamma, Kf.inv_sin2_half_ap), v);
    }
}

// Spectral disc term of frame k for the channel pair (lo, lo + 1, f) added to the sky value o
template <bool FAST>
__device__ __forceinline__ float seq_disc_spec(const SunskyKArgs& K, const SeqArgs& A, int k, const DirTerms& t,
                                               int lo, float f, float o) {
    const SunskyKArgs& Kf = opaque_kargs(K);
    seq_cfloat_p rec = seq_record(A.frames, kNbWavelengths, seq_opaque(k));
    const RadianceStage rs = seq_sun_stage(rec);
    const float* ds = A.sun_rad_ds;
    const int block = A.sun_block;
    const int hi = lo + 1;
    if constexpr (FAST) {   // add_sun_spec64
        const SunDisc64 d = seq_sun_disc64(Kf, mk3(rec[0], rec[1], rec[2]), t.wx, t.wy, t.cos_theta);
        const double fd = (double)f;
        auto poly = [&](int c) {
            const int q = (d.pos * kNbWavelengths + c) * kNbSunCtrlPts;
            return fma(fma(fma((double)sun_param(ds, block, q + 3, rs), d.x, (double)sun_param(ds, block, q + 2, rs)), d.x,
                           (double)sun_param(ds, block, q + 1, rs)), d.x, (double)sun_param(ds, block, q, rs));
        };
        double sun = poly(lo);
        if (f != 0.f) sun = fma(fd, (hi < kNbWavelengths ? poly(hi) : 0.0) - sun, sun);
        double ld = 0.0;
#pragma unroll 1
        for (int j = kNbSunLdParams - 1; j >= 0; --j) {
            double coef = (double)Kf.sun_ld[lo * kNbSunLdParams + j];
            if (f != 0.f) coef = fma(fd, (hi < kNbWavelengths ? (double)Kf.sun_ld[hi * kNbSunLdParams + j] : 0.0) - coef, coef);
            ld = fma(ld, d.cpsi, coef);
        }
        return (float)fma((double)Kf.sun_mul, sun * ld, (double)o);
    } else {
        float xs;
        const int pos = seq_segment_ref(Kf, t.cos_theta, &xs);
        return seq_disc_spec_at(Kf, ds, block, rs, pos, xs, cos_psi(t.gamma, Kf.inv_sin2_half_ap), lo, f, o);
    }
}

// Direction sources: a ray batch (eval: wo = -wi) or the lat-long grid of bake_latlong
struct SeqRays {
    const float *wx, *wy, *wz;
    const uint8_t* active;
    __device__ __forceinline__ float3_ local_dir(const SunskyKArgs& K, size_t i, bool* m) const {
        *m = !active || active[i] != 0;
        return to_local(K, flip3<true>(wx[i], wy[i], wz[i]));
    }
};
struct SeqGrid {
    LatLong G;
    __device__ __forceinline__ float3_ local_dir(const SunskyKArgs& K, size_t i, bool* m) const {
        *m = true;
        return to_local(K, latlong_dir(G, i));
    }
};

template <bool FAST, class SRC>
__device__ __forceinline__ void seq_rgb_body(const SunskyKArgs& K, const SeqArgs& A, const SRC& src, size_t n,
                                             float* __restrict__ out, size_t ostride) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int chans[3] = {0, 1, 2};
    const int count = A.count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        bool m;
        const float3_ wo = src.local_dir(K, i, &m);
        const SeqDir s = seq_dir<FAST>(wo, m);
        float acc[3] = {0.f, 0.f, 0.f};
        SeqHot<FAST, 3> cur = seq_load<FAST, 3>(A.frames, 3, 0, chans);
#pragma unroll 1
        for (int k = 0; k < count; ++k) {
            // the next record's scalar loads, in flight under this frame's arithmetic
            const SeqHot<FAST, 3> nxt = seq_load<FAST, 3>(A.frames, 3, k + 1 < count ? k + 1 : k, chans);
            const DirTerms t = seq_frame_terms<FAST>(s, cur.sn, K.cos_cutoff);
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = sky_eval<FAST>(cur.ch[c], t, K.sky_scale);
            if (t.hit_sun) seq_disc_rgb<FAST>(K, A, k, t, v);
            if constexpr (!FAST) {
                const float cie = (float)kCieYNormalization;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = v[c] * cie;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = fmaf(cur.w, v[c], acc[c]);
            cur = nxt;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) store_nt(s.active ? acc[c] : 0.f, out + (size_t)c * ostride + i);
    }
}

// Spectral, one broadcast wavelength list: per output wavelength the frame loop over its
// channel pair (the disc term is not linear in the nodes, so nothing is shared between
// wavelengths but the direction's frame-independent terms)
template <bool FAST, class SRC>
__device__ __forceinline__ void seq_spec_body(const SunskyKArgs& K, const SeqArgs& A, const LambdaSet& L,
                                              const SRC& src, size_t n, float* __restrict__ out, size_t ostride) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int count = A.count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        bool m;
        const float3_ wo = src.local_dir(K, i, &m);
        const SeqDir s = seq_dir<FAST>(wo, m);
#pragma unroll 1
        for (int q = 0; q < L.m; ++q) {
            const int lo = L.lo[q];
            const float f = L.f[q];
            float acc = 0.f;
            if (f >= 0.f) {
                const int chans[2] = {lo, lo + 1 < kNbWavelengths ? lo + 1 : lo};
                SeqHot<FAST, 2> cur = seq_load<FAST, 2>(A.frames, kNbWavelengths, 0, chans);
#pragma unroll 1
                for (int k = 0; k < count; ++k) {
                    const SeqHot<FAST, 2> nxt =
                        seq_load<FAST, 2>(A.frames, kNbWavelengths, k + 1 < count ? k + 1 : k, chans);
                    const DirTerms t = seq_frame_terms<FAST>(s, cur.sn, K.cos_cutoff);
                    float v = sky_eval<FAST>(cur.ch[0], t, K.sky_scale);
                    if (f != 0.f) v = lerpf_(v, sky_eval<FAST>(cur.ch[1], t, K.sky_scale), f);
                    if (t.hit_sun) v = seq_disc_spec<FAST>(K, A, k, t, lo, f, v);
                    acc = fmaf(cur.w, v, acc);
                    cur = nxt;
                }
            }
            store_nt(f >= 0.f && s.active ? acc : 0.f, out + (size_t)q * ostride + i);
        }
    }
}

#define SS_SEQUENCE(SUFFIX, FAST)                                                                              \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_eval_rgb##SUFFIX(                   \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, const float* wx, const float* wy, const float* wz,      \
        const uint8_t* active, size_t n, float* out, size_t ostride) {                                         \
        seq_rgb_body<FAST>(*Kp, A, SeqRays{wx, wy, wz, active}, n, out, ostride);                              \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_eval_spec##SUFFIX(                  \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, LambdaSet L, const float* wx, const float* wy,          \
        const float* wz, const uint8_t* active, size_t n, float* out, size_t ostride) {                        \
        seq_spec_body<FAST>(*Kp, A, L, SeqRays{wx, wy, wz, active}, n, out, ostride);                          \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_bake_rgb##SUFFIX(                   \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, LatLong G, float* out, size_t ostride) {                \
        seq_rgb_body<FAST>(*Kp, A, SeqGrid{G}, (size_t)G.w * (size_t)G.h, out, ostride);                       \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_bake_spec##SUFFIX(                  \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, LatLong G, LambdaSet L, float* out, size_t ostride) {   \
        seq_spec_body<FAST>(*Kp, A, L, SeqGrid{G}, (size_t)G.w * (size_t)G.h, out, ostride);                   \
    }
SS_SEQUENCE(_fast, true)
SS_SEQUENCE(_ref, false)

// Shared by the sampling and irradiance parts (sequence_sampling.h, sequence_irradiance*.h).
// One frame's term sky_k(s), unweighted, of the record `cur`: what seq_sky_sum weighs and adds,
// and what sunsky_sequence_irradiance_grad_fold contracts with the adjoint image.  Reference
// precision, the disc branch off.  RGB = true: N = 3 planes, each x MI_CIE_Y_NORMALIZATION.
// Otherwise one plane: channel c[0], or (N = 2) the lerp of c[0] and c[1] by f != 0, as
// seq_spec_body forms a wavelength between two nodes.
template <bool RGB, int N>
__device__ __forceinline__ void seq_sky_frame(const SunskyKArgs& K, const SeqHot<false, N>& cur, const SeqDir& s, float f,
                                              float (&v)[RGB ? 3 : 1]) {
    static_assert(RGB ? N == 3 : (N == 1 || N == 2), "3 RGB planes, or one plane from one or two nodes");
    const DirTerms t = seq_frame_terms<false>(s, cur.sn, K.cos_cutoff);
    if constexpr (RGB) {
        const float cie = (float)kCieYNormalization;
#pragma unroll
        for (int p = 0; p < 3; ++p) v[p] = sky_eval<false>(cur.ch[p], t, K.sky_scale) * cie;
    } else {
        v[0] = sky_eval<false>(cur.ch[0], t, K.sky_scale);
        if constexpr (N == 2)
            if (f != 0.f) v[0] = lerpf_(v[0], sky_eval<false>(cur.ch[1], t, K.sky_scale), f);
    }
}

// The frame loop of the sky tables (sunsky_sequence_table, sunsky_sequence_irradiance_table):
// sum_k w_k sky_k(s) of the N channels c[], added in frame order as fma(w_k, v, acc).
template <bool RGB, int N>
__device__ __forceinline__ void seq_sky_sum(const SunskyKArgs& K, const SeqArgs& A, const SeqDir& s, const int (&c)[N],
                                            float f, float (&acc)[RGB ? 3 : 1]) {
    const int nch = RGB ? 3 : kNbWavelengths, count = A.count;
#pragma unroll
    for (int p = 0; p < (RGB ? 3 : 1); ++p) acc[p] = 0.f;
    SeqHot<false, N> cur = seq_load<false, N>(A.frames, nch, 0, c);
#pragma unroll 1
    for (int k = 0; k < count; ++k) {
        const SeqHot<false, N> nxt = seq_load<false, N>(A.frames, nch, k + 1 < count ? k + 1 : k, c);
        float v[RGB ? 3 : 1];
        seq_sky_frame<RGB, N>(K, cur, s, f, v);
#pragma unroll
        for (int p = 0; p < (RGB ? 3 : 1); ++p) acc[p] = fmaf(cur.w, v[p], acc[p]);
        cur = nxt;
    }
}

// Batched staging of a sequence's records: workgroup = frame, sunsky_stage_radiance's sky part
// (radiance_param per entry, then one thread per channel folds it) from the RadianceStage
// scalars the host put into the record's header.  No sun table: see seq_disc_*.
extern "C" __global__ __launch_bounds__(256) void sunsky_stage_sequence(SeqStageArgs A) {
    __shared__ float p[kNbWavelengths * kNbSkyParams];
    __shared__ float r[kNbWavelengths];
    const int t = threadIdx.x;
    const int np = A.nch * kNbSkyParams;
    const size_t rec_bytes = kSeqFrameHeader + (size_t)A.nch * (sizeof(FastChannel) + sizeof(SkyChannel));
    for (int fr = blockIdx.x; fr < A.count; fr += gridDim.x) {
        char* rec = static_cast<char*>(A.frames) + (size_t)fr * rec_bytes;
        const SeqFrame<1>* h = reinterpret_cast<const SeqFrame<1>*>(rec);   // the header is the same for every NCH
        RadianceStage rs;
        rs.x = h->x;
        rs.t_rem = h->t_rem;
        rs.t_low = h->t_low;
        rs.t_high = h->t_high;
        rs.in_range = h->in_range;
        for (int e = t; e < np; e += blockDim.x)
            p[e] = radiance_param(A.sky_params_ds, np, e, rs, A.albedo[e / kNbSkyParams]);
        for (int e = t; e < A.nch; e += blockDim.x) r[e] = radiance_param(A.sky_rad_ds, A.nch, e, rs, A.albedo[e]);
        __syncthreads();
        if (t < A.nch) {
            SkyChannel ch;
            FastChannel f;
            fold_channel(&p[t * kNbSkyParams], r[t], A.variant, A.sky_scale, &ch, &f);
            reinterpret_cast<FastChannel*>(rec + kSeqFrameHeader)[t] = f;
            reinterpret_cast<SkyChannel*>(rec + kSeqFrameHeader + (size_t)A.nch * sizeof(FastChannel))[t] = ch;
        }
        __syncthreads();
    }
}
