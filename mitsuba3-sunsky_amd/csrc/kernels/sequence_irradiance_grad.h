// kernels/sequence_irradiance_grad.h -- frame sequences: gradients of the irradiance (receiver normals, frame weights).
// A part of sunsky_kernels.hip (one translation unit): included there, once, in order.

// ======================================================================
// Gradients of the irradiance (sunsky_sequence_irradiance_vjp; the definition is in sunsky_amd.h).
// Normals: seq_irr_pass's loop with the clamp's step in place of the clamp, one launch.  Weights:
// the adjoint image (receivers streamed against the cells and suns a lane owns), then the fold.
// ======================================================================

// One pass over the staged image for a lane's two receivers: g_l = sum over records of
// [n_l . d > 0] (sum_p d_out[p] value_p) d.  NP: the planes held in registers (RGB: 3; spectral:
// the power of two at or above `planes`, the planes beyond it skipped by a wave-uniform test).
// The order is the contract, seq_irr_pass's: a row's cells in column order into a row sum that
// starts at 0, the row sums in row order, then the suns of the image; per record the plane fold
// starts at 0 and runs in plane order; every product-and-add is one fma.
template <bool RGB, int NP, int REC>
__device__ __forceinline__ void seq_irr_vjp_pass(const SeqIrradiance& S, int rec, seq_f2 nx, seq_f2 ny, seq_f2 nz,
                                                 const seq_f2 (&d)[NP], seq_f2 (&g)[3]) {
    if constexpr (REC != 0) rec = REC;
    const int planes = RGB ? 3 : S.planes;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    seq_cfloat_p r = (seq_cfloat_p)__builtin_assume_aligned(S.cells, 16) + 3;
    seq_cfloat_p u = (seq_cfloat_p)__builtin_assume_aligned(S.suns, 16) + 3;
#pragma clang diagnostic pop
    const seq_f2 zero = {0.f, 0.f};
    auto add = [&](seq_cfloat_p q, seq_f2 (&sum)[3]) {
        const seq_f2 dt = seq_fma2(nz, q[-1], seq_fma2(ny, q[-2], nx * q[-3]));
        seq_f2 a = zero;
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (RGB || p < planes) a = seq_fma2(d[p], q[p], a);
        const seq_f2 m = {dt[0] > 0.f ? a[0] : 0.f, dt[1] > 0.f ? a[1] : 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = seq_fma2(m, q[c - 3], sum[c]);
    };
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = zero;
#pragma unroll 1
    for (int i = 0; i < S.nz; ++i) {
        seq_f2 row[3] = {zero, zero, zero};
#pragma unroll 4
        for (int j = 0; j < S.nphi; ++j, r += rec) add(r, row);
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] += row[c];
    }
#pragma unroll 1
    for (int k = 0; k < S.nsuns; ++k, u += rec) add(u, g);
}

// Two receivers per lane, as seq_irradiance_body pairs them; the masked cotangent of both in
// registers (a masked lane's is 0 and its gradient is stored as exact zeros).
template <bool RGB, int NP>
__device__ __forceinline__ void seq_irr_vjp_normal_planes(const SunskyKArgs& K, const SeqIrradiance& S, const float* nx,
                                                          const float* ny, const float* nz, const uint8_t* active,
                                                          size_t n, const float* __restrict__ dout, size_t dstride,
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
        seq_f2 g[3];
        seq_irr_vjp_pass<RGB, NP, RGB ? seq_irr_record(3) : 0>(S, seq_irr_record(planes), lx, ly, lz, d, g);
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
__device__ __forceinline__ void seq_irr_vjp_normal_body(const SunskyKArgs& K, const SeqIrradiance& S, const float* nx,
                                                        const float* ny, const float* nz, const uint8_t* active, size_t n,
                                                        const float* dout, size_t dstride, float* gx, float* gy,
                                                        float* gz) {
    if constexpr (RGB) {
        seq_irr_vjp_normal_planes<true, 3>(K, S, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
    } else {
        if (S.planes <= 4) seq_irr_vjp_normal_planes<false, 4>(K, S, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
        else if (S.planes <= 8) seq_irr_vjp_normal_planes<false, 8>(K, S, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
        else if (S.planes <= 16) seq_irr_vjp_normal_planes<false, 16>(K, S, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
        else seq_irr_vjp_normal_planes<false, kSeqIrrMaxPlanes>(K, S, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);
    }
}

// The adjoint image of one slice of receivers: per entry e (cell e < cells, else the sun of
// frame e - cells) and plane p,  rows[slice][p][e] = sum over the slice's receivers of
// d_out[p, r] max(0, n_l,r . dir_e).  Work item = (slice, tile of kSeqIrrGradTile entries, pass
// of NP planes), grid-stride over the items: what an item computes does not depend on the grid.
// A lane owns kSeqIrrGradCellsPerLane entries (e = tile start + c 256 + lane).  The receivers
// are the streamed operand: a chunk of 256, one per lane -- n_l = to_local(n) (the forward's
// bits) and the masked cotangent, all 0 for a masked lane -- goes to LDS once and every lane
// reads it back with one address per wave (a broadcast).  Fixed order: a chunk's receivers in
// index order into a chunk sum that starts at 0, the chunk sums in chunk order into the slice's
// sum; the dot product is the forward's.
template <bool RGB>
__device__ __forceinline__ void seq_irr_adjoint_body(const SunskyKArgs& K, const SeqIrradiance& S, const SeqIrrGrad& G,
                                                     const float* nx, const float* ny, const float* nz,
                                                     const uint8_t* active, size_t n) {
    constexpr int NP = RGB ? 3 : kSeqIrrGradSpecPlanes, CPL = kSeqIrrGradCellsPerLane;
    static_assert(CPL % 2 == 0, "entries go in pairs");
    static_assert(NP + 3 <= 8, "a receiver's LDS record is 8 floats");
    __shared__ float4 sh[kSeqIrrGradChunk][2];   // {n_l.xyz, d[0]}, {d[1], d[2], d[3], -}
    const int tid = threadIdx.x, planes = RGB ? 3 : S.planes, rec = seq_irr_record(planes);
    const size_t cells = (size_t)S.nz * (size_t)S.nphi, entries = cells + (size_t)G.count;
    const size_t tiles = (entries + kSeqIrrGradTile - 1) / kSeqIrrGradTile;
    const size_t passes = (size_t)((planes + NP - 1) / NP);
    const size_t items = (size_t)G.slices * tiles * passes;
    for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int p0 = (int)(item % passes) * NP;
        const size_t tile = (item / passes) % tiles, slice = item / passes / tiles;
        seq_f2 dx[CPL / 2], dy[CPL / 2], dz[CPL / 2];   // entries 2 c and 2 c + 1 share packed instructions
        size_t e[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            e[c] = tile * kSeqIrrGradTile + (size_t)c * kSeqIrrGradChunk + (size_t)tid;
            const size_t ec = e[c] < entries ? e[c] : 0;
            const float* q = ec < cells ? S.cells + ec * (size_t)rec : G.suns + (ec - cells) * 4;
            dx[c / 2][c % 2] = q[0];
            dy[c / 2][c % 2] = q[1];
            dz[c / 2][c % 2] = q[2];
        }
        const seq_f2 zero = {0.f, 0.f};
        seq_f2 acc[CPL / 2][NP];
#pragma unroll
        for (int c = 0; c < CPL / 2; ++c)
#pragma unroll
            for (int p = 0; p < NP; ++p) acc[c][p] = zero;
        const size_t r0 = slice * (size_t)G.slice_len, r1 = r0 + G.slice_len < n ? r0 + G.slice_len : n;
#pragma unroll 1
        for (size_t base = r0; base < r1; base += kSeqIrrGradChunk) {
            __syncthreads();   // every lane is done with the previous chunk
            const size_t i = base + (size_t)tid;
            float3_ nl = mk3(0.f, 0.f, 0.f);
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (i < r1 && (!active || active[i] != 0)) {
                nl = to_local(K, mk3(nx[i], ny[i], nz[i]));
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    if (p0 + p < planes) d[p] = G.dout[(size_t)(p0 + p) * G.dstride + i];
            }
            sh[tid][0] = make_float4(nl.x, nl.y, nl.z, d[0]);
            sh[tid][1] = make_float4(d[1], d[2], d[3], 0.f);
            __syncthreads();
            const int cnt = (int)(r1 - base < (size_t)kSeqIrrGradChunk ? r1 - base : (size_t)kSeqIrrGradChunk);
            seq_f2 part[CPL / 2][NP];
#pragma unroll
            for (int c = 0; c < CPL / 2; ++c)
#pragma unroll
                for (int p = 0; p < NP; ++p) part[c][p] = zero;
#pragma unroll 4
            for (int j = 0; j < cnt; ++j) {
                const float4 a = sh[j][0], b = sh[j][1];
                const float dj[4] = {a.w, b.x, b.y, b.z};
#pragma unroll
                for (int c = 0; c < CPL / 2; ++c) {
                    const seq_f2 cs =
                        __builtin_elementwise_max(seq_fma2(dz[c], a.z, seq_fma2(dy[c], a.y, dx[c] * a.x)), zero);
#pragma unroll
                    for (int p = 0; p < NP; ++p) part[c][p] = seq_fma2(cs, dj[p], part[c][p]);
                }
            }
#pragma unroll
            for (int c = 0; c < CPL / 2; ++c)
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

// Phase 0: rows[0] = ((rows[0] + rows[1]) + rows[2]) + ..., the slices in slice order, one
// element per lane.  Phase 1, one workgroup per frame k (grid-stride over the frames):
//   grad_weight[k] += omega sum_p sum_ij G_p[i, j] sky_{k,p}(c_ij) + sum_p H_p[k] F_k[p]
// with sky_{k,p} from seq_sky_frame (the table kernels' frame body).  Fixed shape: a lane adds
// its cells (cell = lane + 256 t, t ascending) into one sum that starts at 0 -- RGB: a cell's
// three planes in plane order; spectral: plane by plane, an invalid wavelength skipped -- every
// step fma(G, sky, sum); then wave_sum's tree, the 4 waves in wave order, times omega; then the
// sun sum, fma(H_p[k], F_k[p], h) from 0 in plane order, added once.  A frame whose sun is
// below the horizon is left alone (+= exactly 0).
__device__ __forceinline__ void seq_irr_grad_fold_body(const SunskyKArgs& K, const SeqArgs& A, const SeqIrradiance& S,
                                                       const SeqIrrGrad& G, const LambdaSet& L, int phase,
                                                       float* __restrict__ grad_weight) {
    const int planes = S.planes;
    const size_t cells = (size_t)S.nz * (size_t)S.nphi, entries = cells + (size_t)G.count;
    if (phase == 0) {
        const size_t total = (size_t)planes * entries, stride = (size_t)gridDim.x * blockDim.x;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
            float v = G.rows[i];
#pragma unroll 1
            for (unsigned s = 1; s < G.slices; ++s) v += G.rows[(size_t)s * total + i];
            G.rows[i] = v;
        }
        return;
    }
    __shared__ float red[SS_BLOCK / 64];
    const int tid = threadIdx.x;
    for (int k = blockIdx.x; k < G.count; k += gridDim.x) {
        seq_cfloat_p rec = seq_record(A.frames, K.nch, k);
        if (!(rec[2] >= 0.f)) continue;   // wave-uniform: the whole workgroup skips a night frame
        float sum = 0.f;
        if (K.variant == kRGB) {
            const int chans[3] = {0, 1, 2};
            const SeqHot<false, 3> cur = seq_load<false, 3>(A.frames, 3, k, chans);
            for (size_t cell = (size_t)tid; cell < cells; cell += SS_BLOCK) {
                const float3_ wo = seq_cell_centre(S.nz, S.nphi, (int)(cell / (size_t)S.nphi), (int)(cell % (size_t)S.nphi));
                float v[3];
                seq_sky_frame<true, 3>(K, cur, seq_dir<false>(wo, true), 0.f, v);
#pragma unroll
                for (int p = 0; p < 3; ++p) sum = fmaf(G.rows[(size_t)p * entries + cell], v[p], sum);
            }
        } else {
#pragma unroll 1
            for (int q = 0; q < planes; ++q) {
                const int lo = L.lo[q];
                const float f = L.f[q];
                if (!(f >= 0.f)) continue;
                const int chans[2] = {lo, lo + 1 < kNbWavelengths ? lo + 1 : lo};
                const SeqHot<false, 2> cur = seq_load<false, 2>(A.frames, kNbWavelengths, k, chans);
                for (size_t cell = (size_t)tid; cell < cells; cell += SS_BLOCK) {
                    const float3_ wo = seq_cell_centre(S.nz, S.nphi, (int)(cell / (size_t)S.nphi), (int)(cell % (size_t)S.nphi));
                    float v[1];
                    seq_sky_frame<false, 2>(K, cur, seq_dir<false>(wo, true), f, v);
                    sum = fmaf(G.rows[(size_t)q * entries + cell], v[0], sum);
                }
            }
        }
        const float w = wave_sum(sum);
        __syncthreads();   // red[] of the previous frame has been read
        if ((tid & 63) == 0) red[tid >> 6] = w;
        __syncthreads();
        if (tid == 0) {
            float t = red[0];
#pragma unroll
            for (int i = 1; i < SS_BLOCK / 64; ++i) t += red[i];
            float h = 0.f;
#pragma unroll 1
            for (int p = 0; p < planes; ++p) h = fmaf(G.rows[(size_t)p * entries + cells + (size_t)k], G.flux[(size_t)p * G.count + k], h);
            grad_weight[k] += G.omega * t + h;
        }
    }
}

// Both precisions' names run the same bodies, as the forward's do
#define SS_SEQUENCE_IRRADIANCE_GRAD(SUFFIX)                                                                    \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_vjp_normal_rgb##SUFFIX(  \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, const float* nx, const float* ny, const float* nz, \
        const uint8_t* active, size_t n, const float* dout, size_t dstride, float* gx, float* gy, float* gz) { \
        seq_irr_vjp_normal_body<true>(*Kp, S, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);               \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_vjp_normal_spec##SUFFIX( \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, const float* nx, const float* ny, const float* nz, \
        const uint8_t* active, size_t n, const float* dout, size_t dstride, float* gx, float* gy, float* gz) { \
        seq_irr_vjp_normal_body<false>(*Kp, S, nx, ny, nz, active, n, dout, dstride, gx, gy, gz);              \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_adjoint##SUFFIX(         \
        const SunskyKArgs* __restrict__ Kp, SeqIrradiance S, SeqIrrGrad G, const float* nx, const float* ny,   \
        const float* nz, const uint8_t* active, size_t n) {                                                    \
        if (Kp->variant == kRGB) seq_irr_adjoint_body<true>(*Kp, S, G, nx, ny, nz, active, n);                 \
        else seq_irr_adjoint_body<false>(*Kp, S, G, nx, ny, nz, active, n);                                    \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_irradiance_grad_fold##SUFFIX(       \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, SeqIrradiance S, SeqIrrGrad G, LambdaSet L, int phase,  \
        float* grad_weight) {                                                                                  \
        seq_irr_grad_fold_body(*Kp, A, S, G, L, phase, grad_weight);                                           \
    }
SS_SEQUENCE_IRRADIANCE_GRAD(_fast)
SS_SEQUENCE_IRRADIANCE_GRAD(_ref)
