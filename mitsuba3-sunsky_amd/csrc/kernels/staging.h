// kernels/staging.h -- device staging of parameters_changed: sunsky_stage_radiance / tangent / quad_*.
// A part of sunsky_kernels.hip (one translation unit): included there, once, in order.

// ======================================================================
// Device staging of parameters_changed (sunsky.cpp:242-285): the radiance tables
// (compute_radiance_params, sunsky.h:158-231; compute_sun_params, :404-419) and the
// JIT sampling weight / wavelength distribution (estimate_sky_sun_ratio,
// sunsky.cpp:772-886) written straight into the emitter's device state, on the
// caller's stream.  The host writes the rest of the state (geometry, TGMM) with an
// async copy just before; launches that follow on the stream see the new state.
// ======================================================================
// One workgroup: every sky coefficient / radiance entry, every sun-table entry, then
// one thread per channel folds it (sunsky_staging.h: the host model's arithmetic).
extern "C" __global__ __launch_bounds__(256) void sunsky_stage_radiance(StageArgs A) {
    __shared__ float p[kNbWavelengths * kNbSkyParams];
    __shared__ float r[kNbWavelengths];
    const int t = threadIdx.x;
    const int np = A.nch * kNbSkyParams;
    for (int e = t; e < np; e += blockDim.x)
        p[e] = radiance_param(A.sky_params_ds, np, e, A.rs, A.albedo[e / kNbSkyParams]);
    for (int e = t; e < A.nch; e += blockDim.x) r[e] = radiance_param(A.sky_rad_ds, A.nch, e, A.rs, A.albedo[e]);
    for (int i = t; i < A.sun_block; i += blockDim.x) A.sun_table[i] = sun_param(A.sun_rad_ds, A.sun_block, i, A.rs);
    __syncthreads();
    if (t < A.nch) {
        SkyChannel ch;
        FastChannel f;
        fold_channel(&p[t * kNbSkyParams], r[t], A.variant, A.sky_scale, &ch, &f);
        A.state->sky[t] = ch;
        A.state->fsky[t] = f;
    }
}

// Tangent tables of eval_jvp / eval_vjp (sunsky_staging.h TangentArgs): one float per
// thread, fp64 Bezier derivatives of the device-resident datasets, the same code as the
// host model's eval_tangent.
extern "C" __global__ __launch_bounds__(256) void sunsky_stage_tangent(TangentArgs A) {
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < A.total; idx += gridDim.x * blockDim.x)
        A.out[idx] = tangent_buffer_value(A, idx);
}

// Workgroup j = quadrature row j, thread i = point (i, j): its direction terms once,
// every channel's sky and sun terms, then a fixed-shape tree reduction over the row's
// points in LDS (deterministic: the same order on every run).
extern "C" __global__ __launch_bounds__(kQuadBlock) void sunsky_stage_quad_points(QuadArgs A) {
    __shared__ float red[2 * kNbWavelengths][kQuadBlock];
    const int j = blockIdx.x, i = threadIdx.x;
    const SunskyKArgs& K = *A.state;
    float as[kNbWavelengths], au[kNbWavelengths];
#pragma unroll
    for (int c = 0; c < kNbWavelengths; ++c) as[c] = au[c] = 0.f;
    if (i < A.nq) {
        const QuadDir d = quad_dir(K, A.qx, A.qw, i, j);
        const float wj = A.qw[j];
#pragma unroll
        for (int c = 0; c < kNbWavelengths; ++c)
            if (c < A.nch) quad_channel(K, K.sun_table, K.sun_ld, d, wj, c, &as[c], &au[c]);
    }
#pragma unroll
    for (int c = 0; c < kNbWavelengths; ++c) {
        red[c][i] = as[c];
        red[kNbWavelengths + c][i] = au[c];
    }
    __syncthreads();
    for (int h = kQuadBlock / 2; h > 0; h >>= 1) {
        if (i < h)
#pragma unroll
            for (int c = 0; c < 2 * kNbWavelengths; ++c) red[c][i] += red[c][i + h];
        __syncthreads();
    }
    if (i < A.nch) {
        A.rows[(size_t)j * A.nch + i] = red[i][0];
        A.rows[(size_t)(A.nq + j) * A.nch + i] = red[kNbWavelengths + i][0];
    }
}

// One workgroup: the row sums to LDS, thread c adds channel c's rows in row order, then
// one thread derives the sampling weight and the wavelength distribution (quad_finish).
extern "C" __global__ __launch_bounds__(256) void sunsky_stage_quad_finish(QuadArgs A) {
    __shared__ float rows[2 * 200 * kNbWavelengths];
    __shared__ float sky[kNbWavelengths], sun[kNbWavelengths];
    const int total = 2 * A.nq * A.nch;
    for (int i = threadIdx.x; i < total; i += blockDim.x) rows[i] = A.rows[i];
    __syncthreads();
    const int c = threadIdx.x;
    if (c < A.nch) {
        float s = 0.f, u = 0.f;
        for (int j = 0; j < A.nq; ++j) {
            s += rows[j * A.nch + c];
            u += rows[(A.nq + j) * A.nch + c];
        }
        sky[c] = s;
        sun[c] = u;
    }
    __syncthreads();
    if (c == 0) {
        const bool ok = quad_finish(A.state, sky, sun, A.cie_y, A.sky_scale, A.sun_scale);
        if (!ok) *A.status = 1;   // sticky until the host reads it back (sync_host)
    }
}
