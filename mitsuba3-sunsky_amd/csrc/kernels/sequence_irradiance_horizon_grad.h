// kernels/sequence_irradiance_horizon_grad.h -- frame sequences: gradients of the irradiance under a horizon profile (normals, weights, the profile).
// A part of sunsky_kernels.hip (one translation unit): included there, once, in order.

// ======================================================================
// Gradients of the irradiance under a horizon profile (sunsky_sequence_irradiance_horizon_vjp;
// the definition is in sunsky_amd.h).  Normals: seq_irr_vjp_pass's loop with the column loop cut
// into the profile's sectors, one launch.  The profile: a kernel of its own over the one partly
// covered row per (receiver, sector).  Weights: the adjoint image with the visible share v per
// (receiver, entry), then sunsky_sequence_irradiance_grad_fold as it is.
// ======================================================================

// One pass over the staged image for a lane's two receivers under their profiles:
//   g_l = sum over cells of [n_l . c > 0] fp32(a v) c + sum over suns of [s.z >= h] [n_l . s > 0] b s
// with a, b the plane folds of seq_irr_vjp_pass and v = clamp(fma(-h, n_z, i + 1), 0, 1), formed
// once per (row, sector) from the lane's two h values, loaded one sector ahead of their use (the
// forward's HZ loop).  The order is seq_irr_vjp_pass's; the only addition is the rounded a v.
template <bool RGB, int NP, int REC>
__device__ __forceinline__ void seq_irr_hz_vjp_pass(const SeqIrradiance& S, const SeqIrrHorizon& Z, int rec, seq_f2 nx,
                                                    seq_f2 ny, seq_f2 nz, const seq_f2 (&d)[NP], size_t e0, size_t e1,
                                                    seq_f2 (&g)[3]) {
    if constexpr (REC != 0) rec = REC;
    const int planes = RGB ? 3 : S.planes;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    seq_cfloat_p r = (seq_cfloat_p)__builtin_assume_aligned(S.cells, 16) + 3;
    seq_cfloat_p u = (seq_cfloat_p)__builtin_assume_aligned(S.suns, 16) + 3;
    seq_cint_p cols = (seq_cint_p)Z.sun_cols;
#pragma clang diagnostic pop
    const seq_f2 zero = {0.f, 0.f}, one = {1.f, 1.f}, fnz = {(float)S.nz, (float)S.nz};
    const int sectors = Z.sectors, len = Z.sector_len;
    // the lane's two h values of sector b
    auto profile = [&](int b) {
        const float* q = Z.h + (size_t)b * Z.stride;
        const seq_f2 h = {q[e0], q[e1]};
        return h;
    };
    auto fold = [&](seq_cfloat_p q) {
        seq_f2 a = zero;
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (RGB || p < planes) a = seq_fma2(d[p], q[p], a);
        return a;
    };
    auto dot = [&](seq_cfloat_p q) { return seq_fma2(nz, q[-1], seq_fma2(ny, q[-2], nx * q[-3])); };
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = zero;
#pragma unroll 1
    for (int i = 0; i < S.nz; ++i) {
        seq_f2 row[3] = {zero, zero, zero};
        const seq_f2 top = {(float)(i + 1), (float)(i + 1)};
        seq_f2 h = profile(0);
#pragma unroll 1
        for (int b = 0; b < sectors; ++b) {
            const seq_f2 next = profile(b + 1 < sectors ? b + 1 : 0);
            const seq_f2 t = __builtin_elementwise_fma(-h, fnz, top);
            const seq_f2 v = __builtin_elementwise_min(__builtin_elementwise_max(t, zero), one);
#pragma unroll 4
            for (int j = 0; j < len; ++j, r += rec) {
                const seq_f2 dt = dot(r);
                const seq_f2 a = fold(r);
                const seq_f2 av = a * v;
                const seq_f2 m = {dt[0] > 0.f ? av[0] : 0.f, dt[1] > 0.f ? av[1] : 0.f};
#pragma unroll
                for (int c = 0; c < 3; ++c) row[c] = seq_fma2(m, r[c - 3], row[c]);
            }
            h = next;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] += row[c];
    }
#pragma unroll 1
    for (int k = 0; k < S.nsuns; ++k, u += rec) {
        const seq_f2 h = profile(cols[k] / len);
        const float sz = u[-1];
        const seq_f2 dt = dot(u);
        const seq_f2 a = fold(u);
        const seq_f2 m = {dt[0] > 0.f && sz >= h[0] ? a[0] : 0.f, dt[1] > 0.f && sz >= h[1] ? a[1] : 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = seq_fma2(m, u[c - 3], g[c]);
    }
}

// Two receivers per lane, as seq_irr_vjp_normal_planes pairs them.  A lane's elements of a
// sector's plane are its receivers' indices (the first one's for a missing second receiver), or
// 0 for a shared profile.
template <bool RGB, int NP>
__device__ __forceinline__ void seq_irr_hz_vjp_normal_planes(const SunskyKArgs& K, const SeqIrradiance& S,
                                                             const SeqIrrHorizon& Z, const float* nx, const float* ny,
                                                             const float* nz, const uint8_t* active, size_t n,
                                                             const float* __restrict__ dout, size_t dstride,
                                                             float* __restrict__ gx, float* __restrict__ gy,
                                                             float* __restrict__ gz) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, pairs = (n + 1) / 2;
    const int planes = RGB ? 3 : S.planes;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < pairs; t += stride) {
        const size_t idx[2] = {t, t + pairs};
        const bool has[2] = {true, idx[1] < n};
        bool m[2];
        float3_ nl[2];
        seq_f2 d[NP];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const size_t i = has[h] ? idx[h] : t;
            m[h] = !active || active[i] != 0;
            nl[h] = to_local(K, mk3(nx[i], ny[i], nz[i]));
#pragma unroll
            for (int p = 0; p < NP; ++p) d[p][h] = (RGB || p < planes) && m[h] ? dout[(size_t)p * dstride + i] : 0.f;
        }
        const seq_f2 lx = {nl[0].x, nl[1].x}, ly = {nl[0].y, nl[1].y}, lz = {nl[0].z, nl[1].z};
        const size_t e0 = Z.per_receiver ? idx[0] : 0, e1 = Z.per_receiver ? (has[1] ? idx[1] : idx[0]) : 0;
        seq_f2 g[3];
        seq_irr_hz_vjp_pass<RGB, NP, RGB ? seq_irr_record(3) : 0>(S, Z, seq_irr_record(planes), lx, ly, lz, d, e0, e1, g);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!has[h]) continue;
            const float3_ w = to_local_transposed(K, mk3(g[0][h], g[1][h], g[2][h]));
            store_nt(m[h] ? w.x : 0.f, gx + idx[h]);
            store_nt(m[h] ? w.y : 0.f, gy + idx[h]);
            store_nt(m[h] ? w.z : 0.f, gz + idx[h]);
        }
    }
}

template <bool RGB>
__device__ __forceinline__ void seq_irr_hz_vjp_normal_body(const SunskyKArgs& K, const SeqIrradiance& S,
                                                           const SeqIrrHorizon& Z, const float* nx, const float* ny,
                                                           const float* nz, const uint8_t* active, size_t n,
                                                           const float* dout, size_t dstride, float* gx, float* gy,
                                                           float* gz) {
    if constexpr (RGB) {
        seq_irr_hz_vjp_normal_planes<true, 3>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
    } else {
        if (S.planes <= 4) seq_irr_hz_vjp_normal_planes<false, 4>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
        else if (S.planes <= 8) seq_irr_hz_vjp_normal_planes<false, 8>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
        else if (S.planes <= 16) seq_irr_hz_vjp_normal_planes<false, 16>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
        else seq_irr_hz_vjp_normal_planes<false, kSeqIrrMaxPlanes>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
    }
}

// The gradient with respect to the profile: one receiver per lane, and per sector only the one
// row with 0 < t < 1 is walked (n x n_phi cells, 1 / n_z of a pass; riding in the normal kernel's
// loop instead was measured and lost: DESIGN.md).  That row
// is i = ceil(h n_z) - 1 in exact arithmetic; the fp32 product is within half an ulp of h n_z, so
// the row is one of floor(h n_z) - 1, .., + 1, and each candidate is put to the definition's own
// test on t = fma(-h, n_z, i + 1).  The row differs from lane to lane, so the records are read
// per lane (not through scalar loads).  The operations and their order are the definition's:
// the forward's dot product, the plane fold from 0, s = fma(max(0, dot), a, s) from 0 in column
// order, s (-(float)n_z); +0 where no row is partly covered or the lane is masked.
template <bool RGB, int NP>
__device__ __forceinline__ void seq_irr_hz_vjp_profile_planes(const SunskyKArgs& K, const SeqIrradiance& S,
                                                              const SeqIrrHorizon& Z, const float* nx, const float* ny,
                                                              const float* nz, const uint8_t* active, size_t n,
                                                              const float* __restrict__ dout, size_t dstride,
                                                              float* __restrict__ gh, size_t ghstride) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int planes = RGB ? 3 : S.planes, rec = RGB ? seq_irr_record(3) : seq_irr_record(planes);
    const int len = Z.sector_len;
    const float fnz = (float)S.nz;
    for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const bool m = !active || active[r] != 0;
        if (!m) {
#pragma unroll 1
            for (int b = 0; b < Z.sectors; ++b) gh[(size_t)b * ghstride + r] = 0.f;
            continue;
        }
        const float3_ nl = to_local(K, mk3(nx[r], ny[r], nz[r]));
        float d[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) d[p] = (RGB || p < planes) ? dout[(size_t)p * dstride + r] : 0.f;
        const size_t e = Z.per_receiver ? r : 0;
#pragma unroll 1
        for (int b = 0; b < Z.sectors; ++b) {
            const float h = Z.h[(size_t)b * Z.stride + e];
            const int at = (int)fminf(fmaxf(h * fnz, 0.f), fnz);   // a NaN: 0
            int row = -1;
#pragma unroll
            for (int c = -1; c <= 1; ++c) {
                const int i = at + c;
                const float t = fmaf(-h, fnz, (float)(i + 1));
                if (i >= 0 && i < S.nz && t > 0.f && t < 1.f) row = i;
            }
            float val = 0.f;
            if (row >= 0) {
                const float* q = S.cells + ((size_t)row * (size_t)S.nphi + (size_t)b * (size_t)len) * (size_t)rec;
                float s = 0.f;
#pragma unroll 2
                for (int j = 0; j < len; ++j, q += rec) {
                    const float dt = fmaf(nl.z, q[2], fmaf(nl.y, q[1], nl.x * q[0]));
                    float a = 0.f;
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        if (RGB || p < planes) a = fmaf(d[p], q[3 + p], a);
                    s = fmaf(fmaxf(dt, 0.f), a, s);
                }
                val = s * -fnz;
            }
            gh[(size_t)b * ghstride + r] = val;
        }
    }
}

template <bool RGB>
__device__ __forceinline__ void seq_irr_hz_vjp_profile_body(const SunskyKArgs& K, const SeqIrradiance& S,
                                                            const SeqIrrHorizon& Z, const float* nx, const float* ny,
                                                            const float* nz, const uint8_t* active, size_t n,
                                                            const float* dout, size_t dstride, float* gh, size_t ghstride) {
    if constexpr (RGB) {
        seq_irr_hz_vjp_profile_planes<true, 3>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gh, ghstride);
    } else {
        if (S.planes <= 4) seq_irr_hz_vjp_profile_planes<false, 4>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gh, ghstride);
        else if (S.planes <= 8) seq_irr_hz_vjp_profile_planes<false, 8>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gh, ghstride);
        else if (S.planes <= 16) seq_irr_hz_vjp_profile_planes<false, 16>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gh, ghstride);
        else seq_irr_hz_vjp_profile_planes<false, kSeqIrrMaxPlanes>(K, S, Z, nx, ny, nz, active, n, dout, dstride, gh, ghstride);
    }
}

// The adjoint image of one slice of receivers under their profiles: per plane p
//   cell (i, j):  rows[slice][p][i n_phi + j]  = sum_r d_out[p, r] fp32(max(0, n_l,r . c_ij) v_r[i, b(j)])
//   frame k:      rows[slice][p][cells + k]    = sum_r d_out[p, r] [s_k.z >= h_r[b_k]] max(0, n_l,r . s_k)
// in seq_irr_adjoint_body's order (a chunk of 256 receivers in index order into a chunk sum from
// 0, the chunk sums in chunk order).  Work item = (slice, unit, pass of NP planes), grid-stride
// over the items.  The units are sector-aware: sector b's cells (row-major within the sector) in
// tiles of 256 PAIRS 2 entries, so that the one h_r[b] a tile needs rides in the free eighth
// float of a receiver's LDS record; after every sector's cell tiles come the tiles of the K suns
// in frame order, whose lanes read h_r[b_k] of their own sun's sector from global memory (few
// distinct addresses per wave: consecutive frames lie in neighbouring sectors).  PAIRS: 2 where
// a sector has more than 512 cells, else 1 (a function of the grid and H; it does not enter the
// bits: which lane or workgroup owns an entry does not change that entry's sum).
template <bool RGB, int PAIRS>
__device__ __forceinline__ void seq_irr_hz_adjoint_body(const SunskyKArgs& K, const SeqIrradiance& S, const SeqIrrGrad& G,
                                                        const SeqIrrHorizon& Z, const float* nx, const float* ny,
                                                        const float* nz, const uint8_t* active, size_t n,
                                                        float4 (*sh)[2]) {
    constexpr int NP = RGB ? 3 : kSeqIrrGradSpecPlanes, CPL = 2 * PAIRS, TILE = kSeqIrrGradChunk * CPL;
    static_assert(NP + 4 <= 8, "a receiver's LDS record is 8 floats: n_l, NP cotangents, h");
    const int tid = threadIdx.x, planes = RGB ? 3 : S.planes, rec = seq_irr_record(planes);
    const int len = Z.sector_len;
    const size_t cells = (size_t)S.nz * (size_t)S.nphi, entries = cells + (size_t)G.count;
    const size_t sector_cells = (size_t)S.nz * (size_t)len;
    const size_t cell_tiles = (sector_cells + TILE - 1) / TILE, sun_tiles = ((size_t)G.count + TILE - 1) / TILE;
    const size_t units = (size_t)Z.sectors * cell_tiles + sun_tiles;
    const size_t passes = (size_t)((planes + NP - 1) / NP);
    const size_t items = (size_t)G.slices * units * passes;
    const size_t hstep = Z.per_receiver ? 1 : 0;
    const seq_f2 zero = {0.f, 0.f}, one = {1.f, 1.f}, fnz = {(float)S.nz, (float)S.nz};
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int p0 = (int)(item % passes) * NP;
        const size_t unit = (item / passes) % units, slice = item / passes / units;
        const bool sun_tile = unit >= (size_t)Z.sectors * cell_tiles;   // uniform over the workgroup
        const size_t sector = unit / cell_tiles;
        const size_t tile = sun_tile ? unit - (size_t)Z.sectors * cell_tiles : unit % cell_tiles;
        seq_f2 dx[PAIRS], dy[PAIRS], dz[PAIRS], top[PAIRS];   // entries 2 c and 2 c + 1 share packed instructions
        const float* hq[CPL];                                 // a sun's sector plane
        size_t e[CPL];                                        // the entry's place in a workspace row; `entries`: none
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const size_t q = tile * TILE + (size_t)c * kSeqIrrGradChunk + (size_t)tid;
            const float* dir;
            float row1 = 0.f;
            hq[c] = Z.h;
            if (sun_tile) {
                const size_t k = q < (size_t)G.count ? q : 0;
                e[c] = q < (size_t)G.count ? cells + q : entries;
                dir = G.suns + k * 4;
                hq[c] = Z.h + (size_t)(Z.sun_cols[k] / len) * Z.stride;
            } else {
                const size_t qc = q < sector_cells ? q : 0;
                const size_t i = qc / (size_t)len, cell = i * (size_t)S.nphi + sector * (size_t)len + qc % (size_t)len;
                e[c] = q < sector_cells ? cell : entries;
                dir = S.cells + cell * (size_t)rec;
                row1 = (float)(i + 1);
            }
            dx[c / 2][c % 2] = dir[0];
            dy[c / 2][c % 2] = dir[1];
            dz[c / 2][c % 2] = dir[2];
            top[c / 2][c % 2] = row1;
        }
        seq_f2 acc[PAIRS][NP];
#pragma unroll
        for (int c = 0; c < PAIRS; ++c)
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[c][p] = zero;
        const size_t r0 = slice * (size_t)G.slice_len, r1 = r0 + G.slice_len < n ? r0 + G.slice_len : n;
#pragma unroll 1
        for (size_t base = r0; base < r1; base += kSeqIrrGradChunk) {
            __syncthreads();   // every lane is done with the previous chunk
            const size_t i = base + (size_t)tid;
            float3_ nl = mk3(0.f, 0.f, 0.f);
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            float hb = 0.f;
            if (i < r1 && (!active || active[i] != 0)) {
                nl = to_local(K, mk3(nx[i], ny[i], nz[i]));
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    if (p0 + p < planes) d[p] = G.dout[(size_t)(p0 + p) * G.dstride + i];
                if (!sun_tile) hb = Z.h[sector * Z.stride + i * hstep];
            }
            sh[tid][0] = make_float4(nl.x, nl.y, nl.z, d[0]);
            sh[tid][1] = make_float4(d[1], d[2], d[3], hb);
            __syncthreads();
            const int cnt = (int)(r1 - base < (size_t)kSeqIrrGradChunk ? r1 - base : (size_t)kSeqIrrGradChunk);
            seq_f2 part[PAIRS][NP];
#pragma unroll
            for (int c = 0; c < PAIRS; ++c)
#pragma unroll
                for (int p = 0; p < NP; ++p) part[c][p] = zero;
            if (!sun_tile) {
#pragma unroll 4
                for (int j = 0; j < cnt; ++j) {
                    const float4 a = sh[j][0], b = sh[j][1];
                    const float dj[4] = {a.w, b.x, b.y, b.z};
                    const seq_f2 nh = {-b.w, -b.w};
#pragma unroll
                    for (int c = 0; c < PAIRS; ++c) {
                        const seq_f2 v = __builtin_elementwise_min(
                            __builtin_elementwise_max(__builtin_elementwise_fma(nh, fnz, top[c]), zero), one);
                        const seq_f2 cs =
                            __builtin_elementwise_max(seq_fma2(dz[c], a.z, seq_fma2(dy[c], a.y, dx[c] * a.x)), zero) * v;
#pragma unroll
                        for (int p = 0; p < NP; ++p) part[c][p] = seq_fma2(cs, dj[p], part[c][p]);
                    }
                }
            } else {
#pragma unroll 4
                for (int j = 0; j < cnt; ++j) {
                    const float4 a = sh[j][0], b = sh[j][1];
                    const float dj[4] = {a.w, b.x, b.y, b.z};
                    const size_t hi = (base + (size_t)j) * hstep;
#pragma unroll
                    for (int c = 0; c < PAIRS; ++c) {
                        seq_f2 cs =
                            __builtin_elementwise_max(seq_fma2(dz[c], a.z, seq_fma2(dy[c], a.y, dx[c] * a.x)), zero);
                        cs[0] = dz[c][0] >= hq[2 * c][hi] ? cs[0] : 0.f;
                        cs[1] = dz[c][1] >= hq[2 * c + 1][hi] ? cs[1] : 0.f;
#pragma unroll
                        for (int p = 0; p < NP; ++p) part[c][p] = seq_fma2(cs, dj[p], part[c][p]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < PAIRS; ++c)
#pragma unroll
                for (int p = 0; p < NP; ++p) acc[c][p] += part[c][p];
        }
#pragma unroll
        for (int c = 0; c < CPL; ++c)
#pragma unroll
            for (int p = 0; p < NP; ++p)
                if (e[c] < entries && p0 + p < planes)
                    G.rows[(slice * (size_t)planes + (size_t)(p0 + p)) * entries + e[c]] = acc[c / 2][p][c % 2];
    }
}

// Both precisions' names run the same bodies, as the forward's do.  The adjoint's widest body (4
// entries per lane) wants 129 VGPRs, one more than 4 waves per SIMD allow: held to 4.
#define SS_SEQ_IRR_HZ_ADJOINT_ATTR __attribute__((amdgpu_waves_per_eu(4)))
#define SS_SEQUENCE_IRRADIANCE_HORIZON_GRAD(SUFFIX)                                                            \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_horizon_vjp_normal_rgb##SUFFIX( \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, SeqIrrHorizon Z, const float* nx, const float* ny, \
        const float* nz, const uint8_t* active, size_t n, const float* dout, size_t dstride, float* gx, float* gy, \
        float* gz) {                                                                                           \
        seq_irr_hz_vjp_normal_body<true>(*Kp, S, Z, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);         \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_horizon_vjp_normal_spec##SUFFIX( \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, SeqIrrHorizon Z, const float* nx, const float* ny, \
        const float* nz, const uint8_t* active, size_t n, const float* dout, size_t dstride, float* gx, float* gy, \
        float* gz) {                                                                                           \
        seq_irr_hz_vjp_normal_body<false>(*Kp, S, Z, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);        \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_horizon_vjp_profile_rgb##SUFFIX( \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, SeqIrrHorizon Z, const float* nx, const float* ny, \
        const float* nz, const uint8_t* active, size_t n, const float* dout, size_t dstride, float* gh,         \
        size_t ghstride) {                                                                                     \
        seq_irr_hz_vjp_profile_body<true>(*Kp, S, Z, nx, ny, nz, active, n, dout, dstride, gh, ghstride);      \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_horizon_vjp_profile_spec##SUFFIX( \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, SeqIrrHorizon Z, const float* nx, const float* ny, \
        const float* nz, const uint8_t* active, size_t n, const float* dout, size_t dstride, float* gh,         \
        size_t ghstride) {                                                                                     \
        seq_irr_hz_vjp_profile_body<false>(*Kp, S, Z, nx, ny, nz, active, n, dout, dstride, gh, ghstride);     \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) SS_SEQ_IRR_HZ_ADJOINT_ATTR                               \
    void sunsky_sequence_irradiance_horizon_adjoint##SUFFIX(                                                   \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, SeqIrrGrad G, SeqIrrHorizon Z, const float* nx,   \
        const float* ny, const float* nz, const uint8_t* active, size_t n) {                                   \
        __shared__ float4 sh[kSeqIrrGradChunk][2];   /* {n_l.xyz, d[0]}, {d[1], d[2], d[3], h[b]}: one for the four bodies */ \
        const bool wide = (size_t)S.nz * (size_t)Z.sector_len > (size_t)kSeqIrrHzGradNarrowCells;              \
        if (Kp->variant == kRGB) {                                                                             \
            if (wide) seq_irr_hz_adjoint_body<true, 2>(*Kp, S, G, Z, nx, ny, nz, active, n, sh);              \
            else seq_irr_hz_adjoint_body<true, 1>(*Kp, S, G, Z, nx, ny, nz, active, n, sh);                   \
        } else {                                                                                               \
            if (wide) seq_irr_hz_adjoint_body<false, 2>(*Kp, S, G, Z, nx, ny, nz, active, n, sh);             \
            else seq_irr_hz_adjoint_body<false, 1>(*Kp, S, G, Z, nx, ny, nz, active, n, sh);                  \
        }                                                                                                      \
    }
SS_SEQUENCE_IRRADIANCE_HORIZON_GRAD(_fast)
SS_SEQUENCE_IRRADIANCE_HORIZON_GRAD(_ref)
