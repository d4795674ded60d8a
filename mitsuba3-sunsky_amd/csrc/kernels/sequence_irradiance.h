// kernels/sequence_irradiance.h -- frame sequences: irradiance on oriented receivers, with and without a horizon profile.
// A part of sunsky_kernels.hip (one translation unit): included there, once, in order.

// ======================================================================
// Irradiance on oriented receivers (sunsky_sequence_prepare_irradiance / _irradiance; the
// definition is in sunsky_amd.h):
//   E_p(n) = sum_i sum_j omega R_p[i, j] max(0, n_l . c_ij) + sum_k w_k F_k[p] max(0, n_l . s_k)
// prepare_irradiance runs the two table kernels below and stages one image of 16-byte aligned
// records (direction, then the weighted plane values: seq_irr_record); the hot path is a
// receiver x record contraction with one receiver per lane.
// ======================================================================

// R_p[i, j] = (sum_k w_k sky_k(c_ij))_p: sunsky_sequence_table's frame loop with the planes
// kept.  One cell per lane; spectral: one pass per requested wavelength (an invalid one: 0).
extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_table(
    const SunskyKArgs* __restrict__ Kp, SeqArgs A, SeqIrrTableArgs T) {
    const SunskyKArgs& K = *Kp;
    const size_t n = (size_t)T.nz * (size_t)T.nphi, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float3_ wo = seq_cell_centre(T.nz, T.nphi, (int)(i / (size_t)T.nphi), (int)(i % (size_t)T.nphi));
        const SeqDir s = seq_dir<false>(wo, true);
        if (K.variant == kRGB) {
            const int chans[3] = {0, 1, 2};
            float acc[3];
            seq_sky_sum<true, 3>(K, A, s, chans, 0.f, acc);
#pragma unroll
            for (int p = 0; p < 3; ++p) T.sky[(size_t)p * n + i] = acc[p];
        } else {
#pragma unroll 1
            for (int q = 0; q < T.planes; ++q) {
                const int lo = T.L.lo[q];
                const float f = T.L.f[q];
                float acc[1] = {0.f};
                if (f >= 0.f) {
                    const int chans[2] = {lo, lo + 1 < kNbWavelengths ? lo + 1 : lo};
                    seq_sky_sum<false, 2>(K, A, s, chans, f, acc);
                }
                T.sky[(size_t)q * n + i] = acc[0];
            }
        }
    }
}

// F_k[p]: frame k's disc term alone integrated over its cone by the 4 x 16 rule
// (seq_flux_point), reference precision.  One wave per frame, lane = point (a, b): the
// direction through Frame(s_k), its cos theta and elevation segment as eval takes them, cos psi
// = u_a as given (not recomputed from the rounded direction, no cone test); 0 below the horizon
// and for a sun below it.  The 64 weighted values are added by wave_sum's fixed tree.
extern "C" __global__ __launch_bounds__(64) void sunsky_sequence_irradiance_flux(const SunskyKArgs* __restrict__ Kp,
                                                                                 SeqArgs A, SeqIrrTableArgs T) {
    const SunskyKArgs& K = *Kp;
    const int lane = threadIdx.x;
    const SeqFluxPoint pt = seq_flux_point(T.sin2_half_ap, lane / kSeqFluxNphi, lane % kSeqFluxNphi);
    const float ring = kTwoPi / (float)kSeqFluxNphi;
    for (int k = blockIdx.x; k < A.count; k += gridDim.x) {
        seq_cfloat_p rec = seq_record(A.frames, K.nch, k);
        const float3_ sn = mk3(rec[0], rec[1], rec[2]);
        const RadianceStage rs = seq_sun_stage(rec);
        float3_ fs, ft;
        coordinate_system(sn, &fs, &ft);
        const float3_ d = frame_to_world(fs, ft, sn, mk3(pt.x, pt.y, pt.z));
        const bool up = sn.z >= 0.f && d.z >= 0.f;
        float xs = 0.f;
        const int pos = up ? seq_segment_ref(K, fminf(d.z, 1.f), &xs) : 0;
        if (K.variant == kRGB) {
            float v[3] = {0.f, 0.f, 0.f};
            if (up) seq_disc_rgb_at(K, A.sun_rad_ds, A.sun_block, rs, pos, xs, pt.u, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float sum = wave_sum(pt.W * (v[c] * (float)kCieYNormalization));
                if (lane == 0) T.flux[(size_t)c * A.count + k] = ring * sum;
            }
        } else {
#pragma unroll 1
            for (int q = 0; q < T.planes; ++q) {
                const int lo = T.L.lo[q];
                const float f = T.L.f[q];
                float v = 0.f;
                if (up && f >= 0.f) v = seq_disc_spec_at(K, A.sun_rad_ds, A.sun_block, rs, pos, xs, pt.u, lo, f, 0.f);
                const float sum = wave_sum(pt.W * v);
                if (lane == 0) T.flux[(size_t)q * A.count + k] = ring * sum;
            }
        }
    }
}

// Two receivers per lane: every operation of the contraction is one packed fp32 instruction
// over the pair (the record's scalar broadcast to both halves), except the clamp.
typedef float seq_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ seq_f2 seq_fma2(seq_f2 a, float b, seq_f2 c) {
    const seq_f2 bb = {b, b};
    return __builtin_elementwise_fma(a, bb, c);
}

// One pass of the contraction for the NP planes [p0, p0 + NP) of a lane's two receivers with
// local normals (nx, ny, nz)[0 / 1].  The records are read through the constant address space
// with one address per wave (scalar loads into SGPRs, REC floats apart; REC = 0: `rec` at run
// time), so a lane's work per record and receiver is the dot product, the clamp and NP FMAs.
// The order is the contract: a row's cells in column order into a row sum that starts at 0,
// the row sums in row order into the plane's sum, then the suns in list order, every
// product-and-add one fma; the two receivers of a lane never meet.
//
// HZ (sunsky_sequence_irradiance_horizon): the column loop is cut into the profile's
// sectors (their length is wave-uniform).  Per row and sector the lane's two h values, loaded one
// sector ahead of their use, give v = clamp(fma(-h, n_z, i + 1), 0, 1) once; per cell one packed
// multiply (the clamped cosine times v) sits beside the forward's instructions.  A sun counts
// when s_k.z >= h of its column's sector.  h: elements e0 and e1 of the sector's plane in global
// memory (coalesced over receivers; one address for a shared profile), read again in every row
// and served by the caches (a copy per lane in LDS was measured and lost: DESIGN.md).
// The cell loop is unrolled by 4 records; passes of more than 8 planes (the per-frame series')
// by SS_SEQ_IRR_WIDE_UNROLL = 2: four 112-byte records want more scalar registers than there are
// (measured against 4 and 1: profiles/HISTORY.md).
#define SS_SEQ_IRR_WIDE_UNROLL 2
template <int NP, int REC, bool HZ = false>
__device__ __forceinline__ void seq_irr_pass(const SeqIrradiance& S, int rec, int p0, seq_f2 nx, seq_f2 ny, seq_f2 nz,
                                             seq_f2 (&acc)[NP], const SeqIrrHorizon* Z = nullptr, size_t e0 = 0,
                                             size_t e1 = 0) {
    if constexpr (REC != 0) rec = REC;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    seq_cfloat_p r = (seq_cfloat_p)__builtin_assume_aligned(S.cells, 16) + 3 + p0;
    seq_cfloat_p u = (seq_cfloat_p)__builtin_assume_aligned(S.suns, 16) + 3 + p0;
#pragma clang diagnostic pop
    const seq_f2 zero = {0.f, 0.f};
    // max(0, n . d) for both receivers, d the direction in front of the plane values at q
    auto cosine = [&](seq_cfloat_p q) {
        const seq_f2 d = seq_fma2(nz, q[-1 - p0], seq_fma2(ny, q[-2 - p0], nx * q[-3 - p0]));
        return __builtin_elementwise_max(d, zero);
    };
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = zero;
    if constexpr (HZ) {
        const seq_f2 one = {1.f, 1.f}, fnz = {(float)S.nz, (float)S.nz};
        const int sectors = Z->sectors, len = Z->sector_len;
        // the lane's two h values of sector b
        auto profile = [&](int b) {
            const float* q = Z->h + (size_t)b * Z->stride;
            const seq_f2 h = {q[e0], q[e1]};
            return h;
        };
#pragma unroll 1
        for (int i = 0; i < S.nz; ++i) {
            seq_f2 row[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) row[p] = zero;
            const seq_f2 top = {(float)(i + 1), (float)(i + 1)};
            seq_f2 h = profile(0);
#pragma unroll 1
            for (int b = 0; b < sectors; ++b) {
                const seq_f2 next = profile(b + 1 < sectors ? b + 1 : 0);
                const seq_f2 v = __builtin_elementwise_min(
                    __builtin_elementwise_max(__builtin_elementwise_fma(-h, fnz, top), zero), one);
#pragma unroll NP > 8 ? SS_SEQ_IRR_WIDE_UNROLL : 4
                for (int j = 0; j < len; ++j, r += rec) {
                    const seq_f2 c = cosine(r) * v;
#pragma unroll
                    for (int p = 0; p < NP; ++p) row[p] = seq_fma2(c, r[p], row[p]);
                }
                h = next;
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[p] += row[p];
        }
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        seq_cint_p cols = (seq_cint_p)Z->sun_cols;
#pragma clang diagnostic pop
#pragma unroll 1
        for (int k = 0; k < S.nsuns; ++k, u += rec) {
            const seq_f2 h = profile(cols[k] / len);
            const float sz = u[-1 - p0];
            seq_f2 c = cosine(u);
            c[0] = sz >= h[0] ? c[0] : 0.f;
            c[1] = sz >= h[1] ? c[1] : 0.f;
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[p] = seq_fma2(c, u[p], acc[p]);
        }
        return;
    }
#pragma unroll 1
    for (int i = 0; i < S.nz; ++i) {
        seq_f2 row[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) row[p] = zero;
#pragma unroll NP > 8 ? SS_SEQ_IRR_WIDE_UNROLL : 4
        for (int j = 0; j < S.nphi; ++j, r += rec) {
            const seq_f2 c = cosine(r);
#pragma unroll
            for (int p = 0; p < NP; ++p) row[p] = seq_fma2(c, r[p], row[p]);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] += row[p];
    }
#pragma unroll 1
    for (int k = 0; k < S.nsuns; ++k, u += rec) {
        const seq_f2 c = cosine(u);
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] = seq_fma2(c, u[p], acc[p]);
    }
}

// Two receivers per lane, t and t + ceil(n / 2) (both streams coalesced), grid-stride over the
// pairs.  RGB: one pass of 3 planes over 32-byte records.  Spectral: passes of 8, 4, 2 and 1
// planes (a plane's sum does not depend on the pass it is in).
// HZ: under the horizon profiles Z; a lane's elements of a sector's plane are its receivers'
// indices (the first one's for a missing second receiver), or 0 for a shared profile.
template <bool RGB, bool HZ = false>
__device__ __forceinline__ void seq_irradiance_body(const SunskyKArgs& K, const SeqIrradiance& S, const float* nx,
                                                    const float* ny, const float* nz, const uint8_t* active, size_t n,
                                                    float* __restrict__ out, size_t ostride,
                                                    const SeqIrrHorizon* Z = nullptr) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, pairs = (n + 1) / 2;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < pairs; t += stride) {
        const size_t idx[2] = {t, t + pairs};
        const bool has[2] = {true, idx[1] < n};
        bool m[2];
        float3_ nl[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const size_t i = has[h] ? idx[h] : t;
            m[h] = !active || active[i] != 0;
            nl[h] = to_local(K, mk3(nx[i], ny[i], nz[i]));
        }
        const seq_f2 lx = {nl[0].x, nl[1].x}, ly = {nl[0].y, nl[1].y}, lz = {nl[0].z, nl[1].z};
        auto store = [&](int p, seq_f2 v) {
            store_nt(m[0] ? v[0] : 0.f, out + (size_t)p * ostride + idx[0]);
            if (has[1]) store_nt(m[1] ? v[1] : 0.f, out + (size_t)p * ostride + idx[1]);
        };
        size_t e0 = 0, e1 = 0;
        if constexpr (HZ) {
            e0 = Z->per_receiver ? idx[0] : 0;
            e1 = Z->per_receiver ? (has[1] ? idx[1] : idx[0]) : 0;
        }
        if constexpr (RGB) {
            seq_f2 acc[3];
            seq_irr_pass<3, seq_irr_record(3), HZ>(S, 0, 0, lx, ly, lz, acc, Z, e0, e1);
#pragma unroll
            for (int p = 0; p < 3; ++p) store(p, acc[p]);
        } else {
            const int rec = seq_irr_record(S.planes);
            int p0 = 0;
            auto pass = [&](auto np) {
                constexpr int NP = decltype(np)::value;
                seq_f2 acc[NP];
                seq_irr_pass<NP, 0, HZ>(S, rec, p0, lx, ly, lz, acc, Z, e0, e1);
#pragma unroll
                for (int p = 0; p < NP; ++p) store(p0 + p, acc[p]);
                p0 += NP;
            };
#pragma unroll 1
            while (S.planes - p0 >= 8) pass(std::integral_constant<int, 8>());
            if (S.planes - p0 >= 4) pass(std::integral_constant<int, 4>());
            if (S.planes - p0 >= 2) pass(std::integral_constant<int, 2>());
            if (S.planes - p0 >= 1) pass(std::integral_constant<int, 1>());
        }
    }
}

// Both precisions' names run the same body: the tables are reference precision by definition
#define SS_SEQUENCE_IRRADIANCE(SUFFIX)                                                                         \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_rgb##SUFFIX(             \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, const float* nx, const float* ny, const float* nz, \
        const uint8_t* active, size_t n, float* out, size_t ostride) {                                         \
        seq_irradiance_body<true>(*Kp, S, nx, ny, nz, active, n, out, ostride);                                \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_spec##SUFFIX(            \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, const float* nx, const float* ny, const float* nz, \
        const uint8_t* active, size_t n, float* out, size_t ostride) {                                         \
        seq_irradiance_body<false>(*Kp, S, nx, ny, nz, active, n, out, ostride);                               \
    }
SS_SEQUENCE_IRRADIANCE(_fast)
SS_SEQUENCE_IRRADIANCE(_ref)

// The same under a per-receiver (or one shared) horizon profile: sunsky_sequence_irradiance_horizon
#define SS_SEQUENCE_IRRADIANCE_HORIZON(SUFFIX)                                                                 \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_horizon_rgb##SUFFIX(     \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, SeqIrrHorizon Z, const float* nx, const float* ny, \
        const float* nz, const uint8_t* active, size_t n, float* out, size_t ostride) {                        \
        seq_irradiance_body<true, true>(*Kp, S, nx, ny, nz, active, n, out, ostride, &Z);                      \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_horizon_spec##SUFFIX(    \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, SeqIrrHorizon Z, const float* nx, const float* ny, \
        const float* nz, const uint8_t* active, size_t n, float* out, size_t ostride) {                        \
        seq_irradiance_body<false, true>(*Kp, S, nx, ny, nz, active, n, out, ostride, &Z);                     \
    }
SS_SEQUENCE_IRRADIANCE_HORIZON(_fast)
SS_SEQUENCE_IRRADIANCE_HORIZON(_ref)
