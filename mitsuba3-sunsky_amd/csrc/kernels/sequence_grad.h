// kernels/sequence_grad.h -- frame sequences: per-frame gradients of the weighted sum, and the staging of their records.
// A part of sunsky_kernels.hip (one translation unit): included there, once, in order.

// ======================================================================
// Reverse mode over a sequence (sunsky_sequence_eval_vjp): with the cotangent d_out,
//   grad_weight[k]    += sum_rays sum_planes d_out eval_k
//   grad_turbidity[k] += w_k sum_rays sum_planes d_out d eval_k / d T_k
//   grad_sun_dir[3 k + a] += w_k sum_rays sum_planes d_out d eval_k / d s_k[a]
// in reference-precision arithmetic whatever the sequence's precision (eval_vjp's conventions:
// masks, segments and floor(T) are not differentiated).  One ray per lane in a grid-stride loop
// whose trip count is uniform per workgroup; the direction's frame-independent terms once, then
// the frame loop of seq_rgb_body.  Per frame the terms are the single emitter's (sky_val,
// sky_tan_weights, sky_dot, sky_tan_gamma, unit_angle_tan_*, cos_psi_jvp, the disc polynomial
// and its derivatives) against the frame's gradient record (SeqGradFrame), both read through
// the constant address space with one address per wave; the next frame's header and sun
// tangents are loaded under this frame's arithmetic, a channel's two 10-float tangent rows
// where the channel is evaluated (two frames' rows would not fit the scalar registers).
// Every frame needs its own 5 sums over rays.  A lane folds d eta x (unit-elevation sum) into
// its 3 sun sums and scales by w_k; the wave adds the 5 values by shuffles (wave_sum); lane 0
// adds them to the wave's row [count][5], kept in dynamic LDS while count <= kSeqGradLdsFrames
// (the workgroup then adds its 4 rows in wave order into one row of the workspace at the end),
// otherwise kept in the workspace itself, one row per wave (the first trip stores, later trips
// add: no row is ever cleared).  sunsky_sequence_grad_reduce adds the rows in a fixed order.  No float atomics: two runs give the same bits.
// ======================================================================
__device__ __forceinline__ seq_cfloat_p seq_grad_record(const void* grads, int nch, int k) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    return (seq_cfloat_p)grads + (size_t)k * (size_t)(2 * seq_grad_block(nch) + 12);
#pragma clang diagnostic pop
}

// What the frame loop prefetches of a frame: the record's header and the gradient record's sun tangents
struct SeqGradHot {
    float3_ sn;
    float w;
    float3_ dl[3];
    float deta[3];
};

__device__ __forceinline__ SeqGradHot seq_grad_load(const void* frames, const void* grads, int nch, int k) {
    seq_cfloat_p rec = seq_record(frames, nch, k);
    seq_cfloat_p g = seq_grad_record(grads, nch, k) + 2 * seq_grad_block(nch);
    SeqGradHot h;
    h.sn = mk3(rec[0], rec[1], rec[2]);
    h.w = rec[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        h.dl[a] = mk3(g[3 * a], g[3 * a + 1], g[3 * a + 2]);
        h.deta[a] = g[9 + a];
    }
    return h;
}

// One sky channel's value and reverse-mode terms (sky_side without the albedo tangent): the
// unscaled value, the tangents along turbidity and the unit elevation (d gamma = 0), and the
// gamma part of the sun axes
struct SeqSkySide { float v, t, e, gm; };

__device__ __forceinline__ SeqSkySide seq_sky_side(const SkyChannel& k, seq_cfloat_p dT, seq_cfloat_p dE,
                                                   const DirTerms& t, float sg) {
    const SkyVal s = sky_val(k, t);
    const SkyTanW W = sky_tan_weights(k, t, s);
    float a[10], b[10];
#pragma unroll
    for (int p = 0; p < 10; ++p) { a[p] = dT[p]; b[p] = dE[p]; }
    SeqSkySide r;
    r.v = W.w[9] * k.rad;
    r.t = sky_dot(W, a);
    r.e = sky_dot(W, b);
    r.gm = sky_tan_gamma(k, t, s, sg);
    return r;
}

// RGB disc terms of frame k (the rare branch; seq_disc_rgb<false>'s value, eval_vjp_rgb_body's
// derivatives): the turbidity slope of each table entry on the spot from the raw dataset
// (sun_param_tangent with dT = 1), d cos psi along the 3 sun axes.  g: w, T, s_x, s_y, s_z.
__device__ __forceinline__ void seq_disc_vjp_rgb(const SunskyKArgs& K, const SeqArgs& A, int k, const DirTerms& t,
                                                 float sg, const float dgs[3], const float cot[3],
                                                 float g[kSeqGradSums]) {
    const SunskyKArgs& Kf = opaque_kargs(K);
    seq_cfloat_p rec = seq_record(A.frames, 3, seq_opaque(k));
    const RadianceStage rs = seq_sun_stage(rec);
    TangentStage ts{};
    ts.dT = 1.0;
    ts.t_low = rs.t_low;
    ts.t_high = rs.t_high;
    const float* ds = A.sun_rad_ds;
    const int block = A.sun_block;
    constexpr int per_c = kNbSunCtrlPts * kNbSunLdParams;
    float xs, cp = 0.f, dcps[3];
    const int pos = seq_segment_ref(Kf, t.cos_theta, &xs);
#pragma unroll
    for (int a = 0; a < 3; ++a) cos_psi_jvp(Kf, t, sg, dgs[a], &cp, &dcps[a]);
    const float sc = Kf.sun_scale * Kf.area_ratio * (float)kSpecToRgbSunConv;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        const int base = pos * (3 * per_c) + c * per_c;
        float v = 0.f, dT = 0.f, dC = 0.f;   // value, d / dT, d / d cos psi
#pragma unroll 1
        for (int kk = 0; kk < kNbSunCtrlPts; ++kk)
#pragma unroll 1
            for (int j = 0; j < kNbSunLdParams; ++j) {
                const int e = base + kk * kNbSunLdParams + j;
                const float S = sun_param(ds, block, e, rs), dS = sun_param_tangent(ds, block, e, ts);
                const float xk = powif_(xs, kk);
                v += xk * powif_(cp, j) * S;
                dT += xk * powif_(cp, j) * dS;
                if (j > 0) dC += xk * (float)j * powif_(cp, j - 1) * S;
            }
        const float cs = cot[c] * sc;
        g[0] += cs * v;
        g[1] += cs * dT;
#pragma unroll
        for (int a = 0; a < 3; ++a) g[2 + a] += cs * dC * dcps[a];
    }
}

// Spectral disc terms of frame k for the channel pair (lo, lo + 1, f) and cotangent cot
__device__ __forceinline__ void seq_disc_vjp_spec(const SunskyKArgs& K, const SeqArgs& A, int k, const DirTerms& t,
                                                  float sg, const float dgs[3], int lo, float f, float cot,
                                                  float g[kSeqGradSums]) {
    const SunskyKArgs& Kf = opaque_kargs(K);
    seq_cfloat_p rec = seq_record(A.frames, kNbWavelengths, seq_opaque(k));
    const RadianceStage rs = seq_sun_stage(rec);
    TangentStage ts{};
    ts.dT = 1.0;
    ts.t_low = rs.t_low;
    ts.t_high = rs.t_high;
    const float* ds = A.sun_rad_ds;
    const int block = A.sun_block;
    const int hi = lo + 1;
    float xs, cp = 0.f, dcps[3];
    const int pos = seq_segment_ref(Kf, t.cos_theta, &xs);
#pragma unroll
    for (int a = 0; a < 3; ++a) cos_psi_jvp(Kf, t, sg, dgs[a], &cp, &dcps[a]);
    auto poly = [&](int c, float* d) {
        const int q = (pos * kNbWavelengths + c) * kNbSunCtrlPts;
        float res = 0.f, dres = 0.f;
#pragma unroll
        for (int e = 0; e < kNbSunCtrlPts; ++e) {
            res += powif_(xs, e) * sun_param(ds, block, q + e, rs);
            dres += powif_(xs, e) * sun_param_tangent(ds, block, q + e, ts);
        }
        *d = dres;
        return res;
    };
    float dsun;
    float sun = poly(lo, &dsun);
    if (f != 0.f) {
        float dsb = 0.f;
        const float sb = hi < kNbWavelengths ? poly(hi, &dsb) : 0.f;
        sun = lerpf_(sun, sb, f);
        dsun = lerpf_(dsun, dsb, f);
    }
    const float ld = sun_limb_darkening(Kf.sun_ld, lo, hi, f, cp);
    float dldc = 0.f;
#pragma unroll 1
    for (int j = 1; j < kNbSunLdParams; ++j) {
        const float a = Kf.sun_ld[lo * kNbSunLdParams + j];
        float coef = a;
        if (f != 0.f) coef = lerpf_(a, hi < kNbWavelengths ? Kf.sun_ld[hi * kNbSunLdParams + j] : 0.f, f);
        dldc += (float)j * powif_(cp, j - 1) * coef;
    }
    const float cs = cot * Kf.sun_scale * Kf.area_ratio;
    g[0] += cs * sun * ld;
    g[1] += cs * dsun * ld;
#pragma unroll
    for (int a = 0; a < 3; ++a) g[2 + a] += cs * sun * dldc * dcps[a];
}

// A lane's 5 sums of frame k: the unit-elevation sum folded into the sun axes, the weight on
// the parameter sums, inactive lanes 0; then the wave's sums into its row (lane 0).
__device__ __forceinline__ void seq_grad_accumulate(float g[kSeqGradSums], float ge, const SeqGradHot& h, bool lane_active,
                                                    float* row, int k, bool first) {
#pragma unroll
    for (int a = 0; a < 3; ++a) g[2 + a] = fmaf(h.deta[a], ge, g[2 + a]);
#pragma unroll
    for (int p = 1; p < kSeqGradSums; ++p) g[p] *= h.w;
    float w[kSeqGradSums];
#pragma unroll
    for (int p = 0; p < kSeqGradSums; ++p) w[p] = wave_sum(lane_active ? g[p] : 0.f);
    if ((threadIdx.x & 63) == 0) {
        float* r = row + (size_t)k * kSeqGradSums;
#pragma unroll
        for (int p = 0; p < kSeqGradSums; ++p) r[p] = first ? w[p] : r[p] + w[p];
    }
}

// The rows of a workgroup's waves: dynamic LDS (4 x count x 5 floats) or the workspace
extern __shared__ float seq_grad_lds[];

__device__ __forceinline__ float* seq_grad_row(const SeqGradArgs& G, int count) {
    const size_t wave = threadIdx.x >> 6, len = (size_t)count * kSeqGradSums;
    return G.lds_rows ? seq_grad_lds + wave * len : G.rows + ((size_t)blockIdx.x * (SS_BLOCK / 64) + wave) * len;
}

// LDS rows -> workspace: the 4 waves' rows added in wave order into the workgroup's one row
__device__ __forceinline__ void seq_grad_flush(const SeqGradArgs& G, int count) {
    if (!G.lds_rows) return;
    __syncthreads();
    const size_t len = (size_t)count * kSeqGradSums;
    float* dst = G.rows + (size_t)blockIdx.x * len;
    for (size_t j = threadIdx.x; j < len; j += SS_BLOCK) {
        float acc = seq_grad_lds[j];
#pragma unroll
        for (int w = 1; w < SS_BLOCK / 64; ++w) acc += seq_grad_lds[w * len + j];
        dst[j] = acc;
    }
}

__device__ __forceinline__ void seq_vjp_rgb_body(const SunskyKArgs& K, const SeqArgs& A, const SeqGradArgs& G,
                                                 const float* __restrict__ wx, const float* __restrict__ wy,
                                                 const float* __restrict__ wz, const uint8_t* __restrict__ active,
                                                 size_t n) {
    const int count = A.count;
    float* row = seq_grad_row(G, count);
    const float cie = (float)kCieYNormalization;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    bool first = true;
    // the loop bound is the workgroup's: every lane of a wave takes part in the wave sums
    for (size_t b = (size_t)blockIdx.x * blockDim.x; b < n; b += stride) {
        const size_t i = b + threadIdx.x;
        bool m = false;
        float3_ wo = mk3(0.f, 0.f, 1.f);
        float cot[3] = {0.f, 0.f, 0.f};
        if (i < n) {
            m = !active || active[i] != 0;
            wo = to_local(K, flip3<true>(wx[i], wy[i], wz[i]));
#pragma unroll
            for (int c = 0; c < 3; ++c) cot[c] = G.dout[(size_t)c * G.dstride + i] * cie;
        }
        const SeqDir s = seq_dir<false>(wo, m);
        SeqGradHot cur = seq_grad_load(A.frames, G.grads, 3, 0);
#pragma unroll 1
        for (int k = 0; k < count; ++k) {
            const SeqGradHot nxt = seq_grad_load(A.frames, G.grads, 3, k + 1 < count ? k + 1 : k);
            const DirTerms t = seq_frame_terms<false>(s, cur.sn, K.cos_cutoff);
            const float sg = sin_gamma(t);
            const UnitAngleTan ua = unit_angle_tan_setup(cur.sn, s.wo);
            float dgs[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) dgs[a] = unit_angle_tan_apply(ua, cur.dl[a]);
            seq_cfloat_p rec = seq_record(A.frames, 3, k), grec = seq_grad_record(G.grads, 3, k);
            float gw = 0.f, gt = 0.f, ge = 0.f, gm = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const SeqSkySide S = seq_sky_side(seq_chan<false>(rec, 3, c), grec + c * 10,
                                                  grec + seq_grad_block(3) + c * 10, t, sg);
                const float cs = cot[c] * K.sky_scale;
                gw = fmaf(cs, S.v, gw);
                gt = fmaf(cs, S.t, gt);
                ge = fmaf(cs, S.e, ge);
                gm = fmaf(cs, S.gm, gm);
            }
            float g[kSeqGradSums] = {gw, gt, gm * dgs[0], gm * dgs[1], gm * dgs[2]};
            if (t.hit_sun) seq_disc_vjp_rgb(K, A, k, t, sg, dgs, cot, g);
            seq_grad_accumulate(g, ge, cur, t.active, row, k, first);
            cur = nxt;
        }
        first = false;
    }
    seq_grad_flush(G, count);
}

// Spectral: frames outside, the wavelength list inside, so a frame's direction terms and its
// wave sums are formed once for all planes.  An invalid wavelength adds nothing.
__device__ __forceinline__ void seq_vjp_spec_body(const SunskyKArgs& K, const SeqArgs& A, const SeqGradArgs& G,
                                                  const LambdaSet& L, const float* __restrict__ wx,
                                                  const float* __restrict__ wy, const float* __restrict__ wz,
                                                  const uint8_t* __restrict__ active, size_t n) {
    const int count = A.count;
    float* row = seq_grad_row(G, count);
    constexpr int gb = seq_grad_block(kNbWavelengths);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    bool first = true;
    for (size_t b = (size_t)blockIdx.x * blockDim.x; b < n; b += stride) {
        const size_t i = b + threadIdx.x;
        const bool in = i < n;
        bool m = false;
        float3_ wo = mk3(0.f, 0.f, 1.f);
        if (in) {
            m = !active || active[i] != 0;
            wo = to_local(K, flip3<true>(wx[i], wy[i], wz[i]));
        }
        const SeqDir s = seq_dir<false>(wo, m);
        SeqGradHot cur = seq_grad_load(A.frames, G.grads, kNbWavelengths, 0);
#pragma unroll 1
        for (int k = 0; k < count; ++k) {
            const SeqGradHot nxt = seq_grad_load(A.frames, G.grads, kNbWavelengths, k + 1 < count ? k + 1 : k);
            const DirTerms t = seq_frame_terms<false>(s, cur.sn, K.cos_cutoff);
            const float sg = sin_gamma(t);
            const UnitAngleTan ua = unit_angle_tan_setup(cur.sn, s.wo);
            float dgs[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) dgs[a] = unit_angle_tan_apply(ua, cur.dl[a]);
            seq_cfloat_p rec = seq_record(A.frames, kNbWavelengths, k), grec = seq_grad_record(G.grads, kNbWavelengths, k);
            float g[kSeqGradSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
            float ge = 0.f, gm = 0.f;
#pragma unroll 1
            for (int q = 0; q < L.m; ++q) {
                const int lo = L.lo[q];
                const float f = L.f[q];
                if (f < 0.f) continue;
                const float cot = in ? G.dout[(size_t)q * G.dstride + i] : 0.f;
                const float wlo = f != 0.f ? 1.f - f : 1.f;   // lerp weights (f = 0: the low channel only)
                const SeqSkySide S = seq_sky_side(seq_chan<false>(rec, kNbWavelengths, lo), grec + lo * 10,
                                                  grec + gb + lo * 10, t, sg);
                float v = wlo * S.v, dt = wlo * S.t, de = wlo * S.e, dm = wlo * S.gm;
                if (f != 0.f) {   // f != 0 means lo <= 9: the high channel exists
                    const SeqSkySide H = seq_sky_side(seq_chan<false>(rec, kNbWavelengths, lo + 1), grec + (lo + 1) * 10,
                                                      grec + gb + (lo + 1) * 10, t, sg);
                    v = fmaf(f, H.v, v);
                    dt = fmaf(f, H.t, dt);
                    de = fmaf(f, H.e, de);
                    dm = fmaf(f, H.gm, dm);
                }
                const float cs = cot * K.sky_scale;
                g[0] = fmaf(cs, v, g[0]);
                g[1] = fmaf(cs, dt, g[1]);
                ge = fmaf(cs, de, ge);
                gm = fmaf(cs, dm, gm);
                if (t.hit_sun) seq_disc_vjp_spec(K, A, k, t, sg, dgs, lo, f, cot, g);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) g[2 + a] = fmaf(gm, dgs[a], g[2 + a]);
            seq_grad_accumulate(g, ge, cur, t.active, row, k, first);
            cur = nxt;
        }
        first = false;
    }
    seq_grad_flush(G, count);
}

// Both names of each kernel (the launch layer's table loads name_fast and name_ref from both
// code objects) run the one reference-precision body: the gradient has no FAST form.
#define SS_SEQUENCE_VJP(SUFFIX)                                                                                \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_eval_vjp_rgb##SUFFIX(               \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, SeqGradArgs G, const float* wx, const float* wy,        \
        const float* wz, const uint8_t* active, size_t n) {                                                    \
        seq_vjp_rgb_body(*Kp, A, G, wx, wy, wz, active, n);                                                    \
    }                                                                                                          \
    extern "C" __global__ __launch_bounds__(SS_BLOCK) void sunsky_sequence_eval_vjp_spec##SUFFIX(              \
        const SunskyKArgs* __restrict__ Kp, SeqArgs A, SeqGradArgs G, LambdaSet L, const float* wx,            \
        const float* wy, const float* wz, const uint8_t* active, size_t n) {                                   \
        seq_vjp_spec_body(*Kp, A, G, L, wx, wy, wz, active, n);                                                \
    }
SS_SEQUENCE_VJP(_fast)
SS_SEQUENCE_VJP(_ref)

// One wave per frame: lane l adds rows l, l + 64, ... in row order, the wave adds the lanes'
// sums (wave_sum), lane 0 accumulates into the outputs that are not NULL.
extern "C" __global__ __launch_bounds__(kSeqGradReduceBlock) void sunsky_sequence_grad_reduce(
    const float* __restrict__ rows, unsigned nrows, int count, float* grad_weight, float* grad_turbidity,
    float* grad_sun_dir) {
    for (int k = blockIdx.x; k < count; k += gridDim.x) {
        float acc[kSeqGradSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (unsigned r = threadIdx.x; r < nrows; r += kSeqGradReduceBlock) {
            const float* p = rows + ((size_t)r * count + k) * kSeqGradSums;
#pragma unroll
            for (int c = 0; c < kSeqGradSums; ++c) acc[c] += p[c];
        }
#pragma unroll
        for (int c = 0; c < kSeqGradSums; ++c) acc[c] = wave_sum(acc[c]);
        if (threadIdx.x == 0) {
            if (grad_weight) grad_weight[k] += acc[0];
            if (grad_turbidity) grad_turbidity[k] += acc[1];
            if (grad_sun_dir)
                for (int a = 0; a < 3; ++a) grad_sun_dir[3 * k + a] += acc[2 + a];
        }
    }
}

// Batched staging of a sequence's gradient records (sunsky_sequence_prepare_grad / _update):
// workgroup = frame, one thread per entry of the two sky blocks, each tangent_value in fp64
// (the function sunsky_stage_tangent runs) with the frame's TangentStage scalars from the
// host: the turbidity tangent (dT = 1) and the unit-elevation tangent (dx = dx / d eta).  The
// host has written dlocal / deta; the blocks' padding is written 0.
extern "C" __global__ __launch_bounds__(256) void sunsky_stage_sequence_grad(SeqGradStageArgs A) {
    __shared__ TangentStage sh[2];
    const int block = seq_grad_block(A.nch), rec = 2 * block + 12;
    for (int fr = blockIdx.x; fr < A.count; fr += gridDim.x) {
        float* g = static_cast<float*>(A.grads) + (size_t)fr * rec;
        if (threadIdx.x < 2) {   // the two tangents in LDS: their albedo is indexed per entry
            TangentStage s = A.stages[fr];
            if (threadIdx.x == 0) s.dT = 1.0;
            else s.dx = s.dx_per_eta;
            sh[threadIdx.x] = s;
        }
        __syncthreads();
        for (int j = threadIdx.x; j < 2 * block; j += blockDim.x) {
            const int e = j % block;
            g[j] = e < A.nch * 10 ? tangent_value(A.sky_params_ds, A.sky_rad_ds, sh[j < block ? 0 : 1], e) : 0.f;
        }
        __syncthreads();
    }
}
