// kernels/sequence_sampling.h -- frame sequences: importance sampling, its sky table and sun list.
// A part of sunsky_kernels.hip (one translation unit): included there, once, in order.

// ======================================================================
// Sequence sampling (sunsky_sequence_sample_direction / _pdf_direction; the distribution is
// SeqSampling's, sunsky_kernel_args.h).  A sample is a sky pick (u1 < w_sky: a row of the table
// from the marginal with u2, a column from the row's distribution with the reused u1, uniform
// within the cell) or a sun pick (a frame from the q distribution with the reused u1, then
// square_to_uniform_cone about that frame's sun, sunsky.cpp:697-701).  Its pdf and the pdf of a
// given direction are ONE function of the local direction: the cell's table value plus
// sum_k q_k [dot(s_k, wo) >= cos_cutoff], the cone test seq_frame_terms makes (hit_sun).  The
// sampler evaluates the weight's numerator with the accumulate loop, so that sum rides along as
// one more accumulator, q_k beside the header's scalar load; the pdf kernel walks 16-byte
// {s_k, q_k} records instead, one address per wave.  Both add in frame order: a sample's
// ds.pdf is bit for bit pdf_direction(ds.d).
// ======================================================================

// First entry of an inclusive normalised CDF above u (entries past the last non-zero one hold
// 1, so u < 1 never reaches them), by bisection: index in [0, n - 1] for every u, NaN included
__device__ __forceinline__ int seq_cdf_search(const float* __restrict__ cdf, int n, float u) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= u) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// sample_reuse: the entry and the position of u within it, in [0, 1)
__device__ __forceinline__ int seq_cdf_sample(const float* __restrict__ cdf, int n, float u, float* reused) {
    const int j = seq_cdf_search(cdf, n, u);
    const float lo = j > 0 ? cdf[j - 1] : 0.f, hi = cdf[j];
    const float t = hi > lo ? (u - lo) / (hi - lo) : 0.f;
    *reused = fminf(fmaxf(t, 0.f), kOneMinusEpsilon);
    return j;
}

// The table value of the cell that holds local direction wo (any wo: the indices are clamped)
__device__ __forceinline__ float seq_sky_cell(const SeqSampling& S, float3_ wo) {
    const int row = (int)fminf(fmaxf(wo.z * (float)S.nz, 0.f), (float)(S.nz - 1));
    float phi = atan2_fast(wo.y, wo.x);
    phi = phi < 0.f ? phi + kTwoPi : phi;
    const int col = (int)fminf(fmaxf(phi * S.inv_dphi, 0.f), (float)(S.nphi - 1));
    return S.f[(size_t)row * (size_t)S.nphi + (size_t)col];
}

__device__ __forceinline__ float seq_pdf_combine(const SeqSampling& S, float fcell, float qsum, bool active) {
    return active ? fmaf(S.sky_coef, fcell, S.sun_coef * qsum) : 0.f;
}

// sum_k q_k [dot(s_k, wo) >= cos_cutoff] over the compact records, in frame order
__device__ __forceinline__ float seq_cone_sum(const float* suns, int count, float3_ wo, float cos_cutoff) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    seq_cfloat_p p = (seq_cfloat_p)suns;
#pragma clang diagnostic pop
    float qsum = 0.f;
#pragma unroll 4
    for (int k = 0; k < count; ++k) {
        const float d = dot3(mk3(p[4 * k], p[4 * k + 1], p[4 * k + 2]), wo);
        qsum += d >= cos_cutoff ? p[4 * k + 3] : 0.f;
    }
    return qsum;
}

// The sample map, in the local frame
template <bool FAST>
__device__ __forceinline__ float3_ seq_sample_local(const SunskyKArgs& K, const SeqSampling& S, int count, float u1,
                                                    float u2) {
    if (u1 < S.w_sky) {
        const float a = fminf(u1 / S.w_sky, kOneMinusEpsilon);
        float t1, t2;
        const int i = seq_cdf_sample(S.row_cdf, S.nz, u2, &t2);
        const int j = seq_cdf_sample(S.cell_cdf + (size_t)i * (size_t)S.nphi, S.nphi, a, &t1);
        const float z = fminf(((float)i + t2) / (float)S.nz, 1.f);
        const float phi = ((float)j + t1) * S.dphi;
        float sp, cp;
        sincos_sel<FAST>(phi, &sp, &cp);
        const float st = safe_sqrt_sel<FAST>(fmaf(-z, z, 1.f));
        return mk3(st * cp, st * sp, z);
    }
    const float a = fminf((u1 - S.w_sky) / (1.f - S.w_sky), kOneMinusEpsilon);
    float t1;
    const int k = seq_cdf_sample(S.frame_cdf, count, a, &t1);
    const float* r = S.suns + 4 * (size_t)k;
    const float3_ sn = mk3(r[0], r[1], r[2]);
    float3_ fs, ft;
    coordinate_system(sn, &fs, &ft);   // Frame3f(local sun), as the emitter's sun_s / sun_t
    float3_ sd = frame_to_world(fs, ft, sn, uniform_cone_dev<FAST>(t1, u2, K.cos_cutoff));
    // cos theta <= 1, as the sky pick's min(): next to the zenith a unit fp32 vector can round to
    // z = 1 + 6e-8, where the disc term's elevation pi/2 - acos(z) is NaN (measured with a sun at
    // 89.9 degrees: a handful of weights per 2^16 zeroed as not finite)
    sd.z = fminf(sd.z, 1.f);
    return sd;
}

// What both samplers do before and beside the frame loop: the sample, ds.d / ds.dist / ds.p
template <bool FAST>
__device__ __forceinline__ SeqDir seq_sample_dir(const SunskyKArgs& K, const SeqSampling& S, int count,
                                                 const SeqSampleIO& io, size_t i) {
    bool act = !io.active || io.active[i] != 0;
    const float3_ sd = seq_sample_local<FAST>(K, S, count, io.ux[i], io.uy[i]);
    act = act && (sd.z >= 0.f);
    const float3_ d = to_world(K, sd);
    store_nt(d.x, io.dx + i);
    store_nt(d.y, io.dy + i);
    store_nt(d.z, io.dz + i);
    if (io.dist || io.opx) {
        const float3_ itp = io.px ? mk3(io.px[i], io.py[i], io.pz[i]) : mk3(0.f, 0.f, 0.f);
        const float3_ rel = mk3(itp.x - K.bs_center[0], itp.y - K.bs_center[1], itp.z - K.bs_center[2]);
        const float dd = 2.f * fmaxf(K.bs_radius, sqrtf(dot3(rel, rel)));
        if (io.dist) store_nt(dd, io.dist + i);
        if (io.opx) {
            store_nt(fmaf(d.x, dd, itp.x), io.opx + i);
            store_nt(fmaf(d.y, dd, itp.y), io.opy + i);
            store_nt(fmaf(d.z, dd, itp.z), io.opz + i);
        }
    }
    // the weight is eval(si{wi = -d}) / pdf at the direction the caller gets: d back in the local frame
    return seq_dir<FAST>(to_local(K, d), act);
}

template <bool FAST>
__device__ __forceinline__ float seq_weight(float e, float pd, float inv_pd, bool active) {
    const float w = FAST ? e * inv_pd : e / pd;
    return active && isfinite(w) ? w : 0.f;
}

template <bool FAST>
__device__ __forceinline__ void seq_sample_rgb_body(const SunskyKArgs& K, const SeqArgs& A, const SeqSampling& S,
                                                    const SeqSampleIO& io, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int chans[3] = {0, 1, 2};
    const int count = A.count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const SeqDir s = seq_sample_dir<FAST>(K, S, count, io, i);
        const float fcell = seq_sky_cell(S, s.wo);
        float acc[3] = {0.f, 0.f, 0.f}, qsum = 0.f;
        // seq_rgb_body's frame loop with the cone sum as a fourth accumulator
        SeqHot<FAST, 3> cur = seq_load<FAST, 3>(A.frames, 3, 0, chans);
        float q = seq_record(A.frames, 3, 0)[kSeqFrameQ];
#pragma unroll 1
        for (int k = 0; k < count; ++k) {
            const int kn = k + 1 < count ? k + 1 : k;
            const SeqHot<FAST, 3> nxt = seq_load<FAST, 3>(A.frames, 3, kn, chans);
            const float qn = seq_record(A.frames, 3, kn)[kSeqFrameQ];
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
            qsum += t.hit_sun ? q : 0.f;
            cur = nxt;
            q = qn;
        }
        const float pd = seq_pdf_combine(S, fcell, qsum, s.active);
        store_nt(pd, io.pdf + i);
        const float inv_pd = fdiv<FAST>(1.f, pd);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            store_nt(seq_weight<FAST>(acc[c], pd, inv_pd, s.active), io.weight + (size_t)c * io.wstride + i);
    }
}

// Spectral: the cone sum rides in the first wavelength's frame loop; a list with no valid
// wavelength takes it from the compact records (the same sum)
template <bool FAST>
__device__ __forceinline__ void seq_sample_spec_body(const SunskyKArgs& K, const SeqArgs& A, const SeqSampling& S,
                                                     const LambdaSet& L, const SeqSampleIO& io, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int count = A.count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const SeqDir s = seq_sample_dir<FAST>(K, S, count, io, i);
        const float fcell = seq_sky_cell(S, s.wo);
        bool have_pd = false;
        float pd = 0.f, inv_pd = 0.f;
#pragma unroll 1
        for (int qi = 0; qi < L.m; ++qi) {
            const int lo = L.lo[qi];
            const float f = L.f[qi];
            float acc = 0.f;
            if (f >= 0.f) {
                float qsum = 0.f;
                const int chans[2] = {lo, lo + 1 < kNbWavelengths ? lo + 1 : lo};
                SeqHot<FAST, 2> cur = seq_load<FAST, 2>(A.frames, kNbWavelengths, 0, chans);
                float q = seq_record(A.frames, kNbWavelengths, 0)[kSeqFrameQ];
#pragma unroll 1
                for (int k = 0; k < count; ++k) {
                    const int kn = k + 1 < count ? k + 1 : k;
                    const SeqHot<FAST, 2> nxt = seq_load<FAST, 2>(A.frames, kNbWavelengths, kn, chans);
                    const float qn = seq_record(A.frames, kNbWavelengths, kn)[kSeqFrameQ];
                    const DirTerms t = seq_frame_terms<FAST>(s, cur.sn, K.cos_cutoff);
                    float v = sky_eval<FAST>(cur.ch[0], t, K.sky_scale);
                    if (f != 0.f) v = lerpf_(v, sky_eval<FAST>(cur.ch[1], t, K.sky_scale), f);
                    if (t.hit_sun) v = seq_disc_spec<FAST>(K, A, k, t, lo, f, v);
                    acc = fmaf(cur.w, v, acc);
                    qsum += t.hit_sun ? q : 0.f;
                    cur = nxt;
                    q = qn;
                }
                if (!have_pd) {
                    pd = seq_pdf_combine(S, fcell, qsum, s.active);
                    inv_pd = fdiv<FAST>(1.f, pd);
                    have_pd = true;
                }
            }
            store_nt(f >= 0.f ? seq_weight<FAST>(acc, pd, inv_pd, s.active) : 0.f, io.weight + (size_t)qi * io.wstride + i);
        }
        if (!have_pd) pd = seq_pdf_combine(S, fcell, seq_cone_sum(S.suns, count, s.wo, K.cos_cutoff), s.active);
        store_nt(pd, io.pdf + i);
    }
}

// pdf_direction: the cell's value and the cone sum; the same in both precisions
__device__ __forceinline__ void seq_pdf_body(const SunskyKArgs& K, const SeqSampling& S, int count, const float* dx,
                                             const float* dy, const float* dz, const uint8_t* active, size_t n,
                                             float* __restrict__ pdf) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const bool m = !active || active[i] != 0;
        const float3_ wo = to_local(K, mk3(dx[i], dy[i], dz[i]));
        const float fcell = seq_sky_cell(S, wo);
        const float qsum = seq_cone_sum(S.suns, count, wo, K.cos_cutoff);
        store_nt(seq_pdf_combine(S, fcell, qsum, m && (wo.z >= 0.f)), pdf + i);
    }
}

#define SS_SEQUENCE_SAMPLING(SUFFIX, FAST)                                                                     \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_sample_rgb##SUFFIX(                 \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, SeqSampling S, SeqSampleIO io, size_t n) {              \
        seq_sample_rgb_body<FAST>(*Kp, A, S, io, n);                                                           \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_sample_spec##SUFFIX(                \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, SeqSampling S, LambdaSet L, SeqSampleIO io, size_t n) { \
        seq_sample_spec_body<FAST>(*Kp, A, S, L, io, n);                                                       \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_pdf##SUFFIX(                        \
        const SunskyKArgs* __restrict__ Kp, SeqSampling S, int count, const float* dx, const float* dy,        \
        const float* dz, const uint8_t* active, size_t n, float* pdf) {                                        \
        seq_pdf_body(*Kp, S, count, dx, dy, dz, active, n, pdf);                                               \
    }
SS_SEQUENCE_SAMPLING(_fast, true)
SS_SEQUENCE_SAMPLING(_ref, false)

// prepare_sampling's table: cell (i, j) = Y(sum_k w_k sky_k(centre)), the accumulate loop in
// reference precision with the disc branch off, one cell per lane.  Y: the RGB luminance
// weights, or sum_c cie_y[c] L_c / 11 over the 11 nodes (quad_finish's).
extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_table(const SunskyKArgs* __restrict__ Kp,
                                                                             SeqArgs A, SeqTableArgs T) {
    const SunskyKArgs& K = *Kp;
    const size_t n = (size_t)T.nz * (size_t)T.nphi, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float3_ wo = seq_cell_centre(T.nz, T.nphi, (int)(i / (size_t)T.nphi), (int)(i % (size_t)T.nphi));
        const SeqDir s = seq_dir<false>(wo, true);
        float y = 0.f;
        if (K.variant == kRGB) {
            const int chans[3] = {0, 1, 2};
            float acc[3];
            seq_sky_sum<true, 3>(K, A, s, chans, 0.f, acc);
            y = luminance_rgb(acc);
        } else {
#pragma unroll 1
            for (int c = 0; c < kNbWavelengths; ++c) {
                const int chans[1] = {c};
                float acc[1];
                seq_sky_sum<false, 1>(K, A, s, chans, 0.f, acc);
                y = fmaf(T.cie_y[c], acc[0], y);
            }
            y = y / (float)kNbWavelengths;
        }
        T.f[i] = fmaxf(y, 0.f);
    }
}

// prepare_sampling's suns: B_k = Y of frame k's disc term alone at the disc centre (what
// seq_disc_* add at wo = s_k), reference precision.  One wave per frame: the disc branch reads
// its record with one address per wave.
extern "C" __global__ __launch_bounds__(64) void sunsky_sequence_suns(const SunskyKArgs* __restrict__ Kp, SeqArgs A,
                                                                      SeqTableArgs T) {
    const SunskyKArgs& K = *Kp;
    for (int k = blockIdx.x; k < A.count; k += gridDim.x) {
        seq_cfloat_p rec = seq_record(A.frames, K.nch, k);
        const float3_ sn = mk3(rec[0], rec[1], rec[2]);
        const DirTerms t = seq_frame_terms<false>(seq_dir<false>(sn, true), sn, K.cos_cutoff);
        float y = 0.f;
        if (t.hit_sun) {
            if (K.variant == kRGB) {
                float v[3] = {0.f, 0.f, 0.f};
                seq_disc_rgb<false>(K, A, k, t, v);
                y = luminance_rgb(v) * (float)kCieYNormalization;
            } else {
#pragma unroll 1
                for (int c = 0; c < kNbWavelengths; ++c) y = fmaf(T.cie_y[c], seq_disc_spec<false>(K, A, k, t, c, 0.f, 0.f), y);
                y = y / (float)kNbWavelengths;
            }
        }
        if (threadIdx.x == 0) T.B[k] = fmaxf(y, 0.f);
    }
}
