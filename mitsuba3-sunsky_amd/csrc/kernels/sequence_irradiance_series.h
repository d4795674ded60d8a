// kernels/sequence_irradiance_series.h -- frame sequences: the per-frame irradiance series.
// A part of sunsky_kernels.hip (one translation unit): included there, once, in order.

// ======================================================================
// Per-frame irradiance series (sunsky_sequence_prepare_irradiance_series / _irradiance_series; the
// definition is in sunsky_amd.h): every frame's own E^k_p(n), bit for bit the irradiance of a
// sequence that holds frame k alone with weight 1.  The frames are staged in groups
// (sunsky_kernel_args.h): a group's image is the forward's image with G * P values per record,
// so one clamped cosine per record and receiver pair is spent on G frames.
// ======================================================================

// A^k_p[i, j] = omega * sky_{k,p}(c_ij) into the groups' images, or sky_{k,p}(c_ij) of one frame
// as a plain table.  One lane per (cell, group), the cell index fastest.  The sky is evaluated at
// the cell centre as sunsky_sequence_irradiance_table computes it on the device; the record's
// direction is the one prepare_irradiance staged from the host.  A frame's value is
// seq_sky_sum's for a sequence of that frame alone with weight 1: fma(1, sky, 0), which gives a
// negative zero the sign the weighted table gives it.
extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_series_table(
    const SunskyKArgs* __restrict__ Kp, SeqArgs A, SeqIrrSeriesTableArgs T) {
    const SunskyKArgs& K = *Kp;
    const size_t cells = (size_t)T.nz * (size_t)T.nphi, n = cells * (size_t)T.groups;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t cell = i % cells;
        const int gr = (int)(i / cells);
        const float3_ wo = seq_cell_centre(T.nz, T.nphi, (int)(cell / (size_t)T.nphi), (int)(cell % (size_t)T.nphi));
        const SeqDir s = seq_dir<false>(wo, true);
        float* rec = T.image ? T.image + ((size_t)gr * cells + cell) * (size_t)T.rec : nullptr;
        if (rec) {   // the direction the forward's image holds (the host's), not this kernel's wo
            const float* c = T.cells + cell * (size_t)T.cells_rec;
            rec[0] = c[0]; rec[1] = c[1]; rec[2] = c[2];
        }
        auto put = [&](int g, int p, float sky) {
            const float v = fmaf(1.f, sky, 0.f);
            if (rec) rec[3 + g * T.planes + p] = T.omega * v;
            else T.raw[(size_t)p * cells + cell] = v;
        };
#pragma unroll 1
        for (int g = 0; g < T.group; ++g) {
            const int k = T.frame0 + gr * T.group + g;
            if (k >= A.count) break;   // past the last frame: the image's zeros stay
            if (K.variant == kRGB) {
                const int chans[3] = {0, 1, 2};
                const SeqHot<false, 3> cur = seq_load<false, 3>(A.frames, 3, k, chans);
                float v[3];
                seq_sky_frame<true, 3>(K, cur, s, 0.f, v);
#pragma unroll
                for (int p = 0; p < 3; ++p) put(g, p, v[p]);
            } else {
#pragma unroll 1
                for (int q = 0; q < T.planes; ++q) {
                    const int lo = T.L.lo[q];
                    const float f = T.L.f[q];
                    float v[1] = {0.f};
                    if (f >= 0.f) {
                        const int chans[2] = {lo, lo + 1 < kNbWavelengths ? lo + 1 : lo};
                        const SeqHot<false, 2> cur = seq_load<false, 2>(A.frames, kNbWavelengths, k, chans);
                        seq_sky_frame<false, 2>(K, cur, s, f, v);
                    }
                    put(g, q, v[0]);
                }
            }
        }
    }
}

// The widest pass of the series' contraction in values (accumulator pairs per lane): 24 takes an
// RGB group in one pass, 16 and 8 were measured against it (profiles/HISTORY.md).  A value's sum
// does not depend on the pass it is in.
#define SS_SEQ_IRR_SERIES_PASS 24

// Work items are (tile of blockDim receiver pairs, group), grid-stride over both with the group
// uniform over the workgroup: its records, suns and columns are read with one address per wave.
// Per item and pass seq_irr_pass runs the sky of NP values over the group's image (no suns of
// its own); then every value takes its frame's one sun, fma(cos, F_k[p], sum), under a horizon
// when s_k.z >= h of the sun's sector; values outside the call's range of frames are not stored
// and a pass without a value in range is skipped.
template <bool RGB, bool HZ>
__device__ __forceinline__ void seq_irr_series_body(const SunskyKArgs& K, const SeqIrrSeries& S, const float* nx,
                                                    const float* ny, const float* nz, const uint8_t* active, size_t n,
                                                    float* __restrict__ out, size_t ostride,
                                                    const SeqIrrHorizon* Z = nullptr) {
    const size_t pairs = (n + 1) / 2, tiles = (pairs + blockDim.x - 1) / blockDim.x;
    const size_t items = tiles * (size_t)S.n_groups;
    const int values = RGB ? 3 * seq_irr_series_group(3) : S.values;
    const int rec = RGB ? seq_irr_record(3 * seq_irr_series_group(3)) : S.rec;
    const seq_f2 zero = {0.f, 0.f};
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int gr = S.group0 + (int)(item / tiles);
        const size_t t = (item % tiles) * blockDim.x + threadIdx.x;
        if (t >= pairs) continue;
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
        size_t e0 = 0, e1 = 0;
        if constexpr (HZ) {
            e0 = Z->per_receiver ? idx[0] : 0;
            e1 = Z->per_receiver ? (has[1] ? idx[1] : idx[0]) : 0;
        }
        const SeqIrradiance C = {S.images + (size_t)gr * S.image_floats, nullptr, S.nz, S.nphi, 0, values};
        const long long base = (long long)gr * values - S.plane0;   // the output plane of the group's value 0
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        seq_cfloat_p suns = (seq_cfloat_p)__builtin_assume_aligned(S.suns, 16) + (size_t)gr * values * 4;
        seq_cint_p cols = (seq_cint_p)S.sun_cols + (size_t)gr * values;
#pragma clang diagnostic pop
        int p0 = 0;
        auto pass = [&](auto np) {
            constexpr int NP = decltype(np)::value;
            const int q0 = p0;
            p0 += NP;
            if (base + q0 + NP <= 0 || base + q0 >= S.n_planes) return;
            seq_f2 acc[NP];
            seq_irr_pass<NP, RGB ? seq_irr_record(3 * seq_irr_series_group(3)) : 0, HZ>(C, rec, q0, lx, ly, lz, acc, Z, e0, e1);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                seq_cfloat_p u = suns + (q0 + p) * 4;
                seq_f2 c = __builtin_elementwise_max(seq_fma2(lz, u[2], seq_fma2(ly, u[1], lx * u[0])), zero);
                if constexpr (HZ) {
                    const float* hq = Z->h + (size_t)(cols[q0 + p] / Z->sector_len) * Z->stride;
                    const float sz = u[2];
                    c[0] = sz >= hq[e0] ? c[0] : 0.f;
                    c[1] = sz >= hq[e1] ? c[1] : 0.f;
                }
                acc[p] = seq_fma2(c, u[3], acc[p]);
                const long long plane = base + q0 + p;
                if (plane < 0 || plane >= S.n_planes) continue;
                float* o = out + (size_t)plane * ostride;
                store_nt(m[0] ? acc[p][0] : 0.f, o + idx[0]);
                if (has[1]) store_nt(m[1] ? acc[p][1] : 0.f, o + idx[1]);
            }
        };
        if constexpr (RGB) {
            constexpr int W = SS_SEQ_IRR_SERIES_PASS, rest = kSeqIrrSeriesWidth % W;
            static_assert(rest == 0 || rest == 8, "an RGB group in passes of W values, then one of 8");
#pragma unroll
            for (int q = 0; q < kSeqIrrSeriesWidth / W; ++q) pass(std::integral_constant<int, W>());
            if constexpr (rest == 8) pass(std::integral_constant<int, 8>());
        } else {
#pragma unroll 1
            while (values - p0 >= SS_SEQ_IRR_SERIES_PASS) pass(std::integral_constant<int, SS_SEQ_IRR_SERIES_PASS>());
            if constexpr (SS_SEQ_IRR_SERIES_PASS > 16)
                if (values - p0 >= 16) pass(std::integral_constant<int, 16>());
            if constexpr (SS_SEQ_IRR_SERIES_PASS > 8)
                if (values - p0 >= 8) pass(std::integral_constant<int, 8>());
            if (values - p0 >= 4) pass(std::integral_constant<int, 4>());
            if (values - p0 >= 2) pass(std::integral_constant<int, 2>());
            if (values - p0 >= 1) pass(std::integral_constant<int, 1>());
        }
    }
}

// Both precisions' names run the same body: the tables are reference precision by definition
#define SS_SEQUENCE_IRRADIANCE_SERIES(SUFFIX)                                                                  \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_series_rgb##SUFFIX(      \
        const SunskyKArgs* __restrict__ Kp, SeqIrrSeries S, const float* nx, const float* ny, const float* nz, \
        const uint8_t* active, size_t n, float* out, size_t ostride) {                                         \
        seq_irr_series_body<true, false>(*Kp, S, nx, ny, nz, active, n, out, ostride);                         \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_series_spec##SUFFIX(     \
        const SunskyKArgs* __restrict__ Kp, SeqIrrSeries S, const float* nx, const float* ny, const float* nz, \
        const uint8_t* active, size_t n, float* out, size_t ostride) {                                         \
        seq_irr_series_body<false, false>(*Kp, S, nx, ny, nz, active, n, out, ostride);                        \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_series_horizon_rgb##SUFFIX( \
        const SunskyKArgs* __restrict__ Kp, SeqIrrSeries S, SeqIrrHorizon Z, const float* nx, const float* ny, \
        const float* nz, const uint8_t* active, size_t n, float* out, size_t ostride) {                        \
        seq_irr_series_body<true, true>(*Kp, S, nx, ny, nz, active, n, out, ostride, &Z);                      \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_series_horizon_spec##SUFFIX( \
        const SunskyKArgs* __restrict__ Kp, SeqIrrSeries S, SeqIrrHorizon Z, const float* nx, const float* ny, \
        const float* nz, const uint8_t* active, size_t n, float* out, size_t ostride) {                        \
        seq_irr_series_body<false, true>(*Kp, S, nx, ny, nz, active, n, out, ostride, &Z);                     \
    }
SS_SEQUENCE_IRRADIANCE_SERIES(_fast)
SS_SEQUENCE_IRRADIANCE_SERIES(_ref)
