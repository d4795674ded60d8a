// sunsky_capi_sequence.cpp -- the frame-sequence half of the C ABI (include/sunsky_amd.h): the
// sequence handle, its host-side staging and table builders, and the sunsky_sequence_* entry
// points.
#include "sunsky_launch.h"

using namespace sunsky;
using namespace sunsky::capi;

// ---------------------------------------------------------------- sequences
// K frames over a snapshot of one emitter (sunsky_amd.h, "frame sequences").  The object
// owns everything its kernels read: a copy of the emitter's state block (geometry, scales,
// aperture, segment thresholds), the frame records, the raw sun dataset the disc lanes lerp
// from, and the limb-darkening table.  Nothing points back to the emitter.
struct sunsky_sequence {
    DrainOnDestroy drain;                    // first: destroyed after every owner below (sunsky_launch.h)
    SunskyKArgs kargs;                       // the snapshot (host); sun_ld -> d_sun_ld on the device
    int count = 0, nch = 0, variant = 0;
    int precision = SUNSKY_PRECISION_FAST;
    int device = -1;                         // -1: host-only (no batch calls)
    DeviceModule* mod = nullptr;
    std::vector<unsigned char> records;      // SeqFrame<nch>[count], staged (host mirror: get_frame)
    size_t rec_bytes = 0;
    int sun_block = 0;
    DeviceBuffer<SunskyKArgs> d_state;
    DeviceBuffer<unsigned char> d_frames;
    DeviceBuffer<float> d_sun_rad, d_sun_ld;
    mutable OrderedScratch<float> bake;      // bake_latlong angle tables, ordered as the emitter's
    // sampling (prepare_sampling): the snapshot's luminance weights and, for host-only
    // sequences, the tables the disc term reads; then the distribution itself
    float cie_y[kNbWavelengths] = {0};
    std::vector<float> h_sun_rad, h_sun_ld;
    int samp_nz = 0, samp_nphi = 0;          // 0: not prepared
    float samp_w_sky = 0.f, samp_sky_mass = 0.f, samp_sun_mass = 0.f;
    std::vector<float> samp_f, samp_row_cdf, samp_cell_cdf, samp_q, samp_frame_cdf, samp_B;
    DeviceBuffer<float> d_samp;              // f, row_cdf, cell_cdf, frame_cdf, suns in one block
    SeqSampling samp = {};
    // what update / prepare_grad restage from: the frames as given (defaults resolved) and the
    // parent's albedo, to_local and raw sky datasets (host copies for host-only sequences, the
    // sequence's own device copy otherwise: the parent may be gone)
    std::vector<float> in_dirs, in_turbidity, in_weights;
    std::vector<float> albedo;
    double to_local_d[9] = {0};
    std::vector<float> h_sky_params_ds, h_sky_rad_ds;
    DeviceBuffer<float> d_sky_ds;            // sky params | sky radiance
    const float *d_sky_params_ds = nullptr, *d_sky_rad_ds = nullptr;
    // gradients (prepare_grad): the records' host mirror (frame_tangent), the device records,
    // the staging scalars and the reduction workspace of the largest grid eval_vjp launches
    bool grad_ready = false;
    std::vector<unsigned char> grads;        // SeqGradFrame<nch>[count]
    DeviceBuffer<unsigned char> d_grads;
    DeviceBuffer<TangentStage> d_grad_stages;
    DeviceBuffer<float> d_grad_rows;
    unsigned grad_max_grid = 0;
    // irradiance (prepare_irradiance): the tables as read back (R_p and F_k[p], unweighted) and
    // the staged device image the hot path walks (cell records, then sun records)
    int irr_nz = 0, irr_nphi = 0, irr_planes = 0;   // 0: not prepared
    float irr_omega = 0.f;
    std::vector<float> irr_sky, irr_flux;
    DeviceBuffer<float> d_irr;
    SeqIrradiance irr = {};
    // the grid column j_k of every frame's sun (irradiance_horizon's sectors); on the device the
    // columns of the image's suns, in the image's order, behind the image
    std::vector<int> irr_sun_cols;
    const int* d_irr_sun_cols = nullptr;
    LambdaSet irr_L = {};                    // the spectral planes' wavelengths (the weight gradient's sky terms)
    // gradients of the irradiance (prepare_irradiance_grad): asked for once (sticky: a later
    // prepare_irradiance restages it), staged for the current tables when irr_grad_ready
    bool irr_grad_wanted = false, irr_grad_ready = false;
    DeviceBuffer<float> d_irr_grad;          // every frame's sun | F_k[p] | every frame's sun column | the reduction workspace
    SeqIrrGrad irr_grad = {};
    const int* d_irr_grad_cols = nullptr;    // the column j_k of all K frames (irradiance_horizon_vjp's adjoint)
    size_t irr_grad_cap = 0;                 // the workspace bound in floats, as read at prepare time
    // the per-frame series (prepare_irradiance_series): sticky as the gradients are; the groups'
    // images, then the values' sun records, then their sun columns in one block
    bool irr_series_wanted = false, irr_series_ready = false;
    DeviceBuffer<float> d_irr_series;
    SeqIrrSeries irr_series = {};
    int irr_series_groups = 0;

    void require_device() const {
        if (!mod) throw std::invalid_argument("host-only sequence (over a sunsky_emitter_create_host emitter) cannot launch kernels");
    }
    void require_grad() const {
        if (!grad_ready)
            throw std::invalid_argument("the sequence has no gradient records yet: call sunsky_sequence_prepare_grad first");
    }
    void require_sampling() const {
        if (!samp_nz)
            throw std::invalid_argument("the sequence has no sampling distribution yet: call "
                                        "sunsky_sequence_prepare_sampling first");
    }
    void require_irradiance() const {
        if (!irr_nz)
            throw std::invalid_argument("the sequence has no irradiance tables yet: call "
                                        "sunsky_sequence_prepare_irradiance first");
    }
    void require_irradiance_grad() const {
        require_irradiance();
        if (!irr_grad_ready)
            throw std::invalid_argument("the sequence's irradiance gradients are not prepared yet: call "
                                        "sunsky_sequence_prepare_irradiance_grad first");
    }
    void require_irradiance_series() const {
        if (!irr_series_ready)
            throw std::invalid_argument("the sequence's irradiance series is not prepared yet: call "
                                        "sunsky_sequence_prepare_irradiance_series first");
    }
    // The snapshot never changes, so an identity to_world takes the identity code object under
    // capture too (SUNSKY_AMD_GENERAL_XFORM=1: the general one always)
    int xform_form(hipStream_t = nullptr) const { return kargs.identity_xform && !general_xform() ? 1 : 0; }
    SeqArgs args() const { return SeqArgs{d_frames.get(), d_sun_rad.get(), count, sun_block}; }

    // the owners free what they hold once this body has run: device current, launches drained
    ~sunsky_sequence() { drain.enter(device); }
};

namespace {

// The header of frame k's record (the same for every channel count)
SeqFrame<1>* seq_header(sunsky_sequence* q, int k) {
    return reinterpret_cast<SeqFrame<1>*>(q->records.data() + (size_t)k * q->rec_bytes);
}
const SeqFrame<1>* seq_header(const sunsky_sequence* q, int k) {
    return reinterpret_cast<const SeqFrame<1>*>(q->records.data() + (size_t)k * q->rec_bytes);
}
const SkyChannel* seq_sky(const sunsky_sequence* q, int k) {
    return reinterpret_cast<const SkyChannel*>(q->records.data() + (size_t)k * q->rec_bytes + kSeqFrameHeader +
                                               (size_t)q->nch * sizeof(FastChannel));
}

// Validation and the per-frame geometry staging from the parent's state: the local sun
// direction as the emitter's constructor forms it (normalised, then to_local; sunsky.cpp:
// 923, 176), and the RadianceStage scalars of (its elevation, the frame's turbidity).
void seq_fill_headers(sunsky_sequence* q, const float* dirs, const float* turbidity, const float* weights) {
    for (int k = 0; k < q->count; ++k) {
        const float T = turbidity[k];
        if (!(T >= 1.f && T <= 10.f)) {
            char buf[128];
            std::snprintf(buf, sizeof(buf), "Turbidity value %f is out of range [1, 10]", T);
            throw std::invalid_argument(std::string(buf) + " (frame " + std::to_string(k) + ")");
        }
        const float w = weights[k];
        if (!std::isfinite(w) || w < 0.f)
            throw std::invalid_argument("frame " + std::to_string(k) + ": the weight must be finite and >= 0");
        const float3_ d = mk3(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
        const float len2 = dot3(d, d);
        if (!std::isfinite(len2) || !(len2 > 0.f))
            throw std::invalid_argument("frame " + std::to_string(k) + ": the sun direction must be finite and non-zero");
        const float inv = 1.f / sqrtf(len2);
        const float3_ l = xform_vec(q->kargs.to_local, mk3(d.x * inv, d.y * inv, d.z * inv));
        const RadianceStage rs = radiance_stage_for(unit_angle_z(l), T);
        SeqFrame<1>* h = seq_header(q, k);
        h->sun_n[0] = l.x; h->sun_n[1] = l.y; h->sun_n[2] = l.z;
        h->weight = w;
        h->t_rem = rs.t_rem;
        h->t_low = rs.t_low;
        h->t_high = rs.t_high;
        h->turbidity = T;
        h->x = rs.x;
        h->in_range = rs.in_range;
    }
}

// sunsky_stage_sequence on the host (host-only sequences): the same functions per entry
void seq_stage_host(sunsky_sequence* q, float sky_scale) {
    const int nch = q->nch, np = nch * kNbSkyParams;
    const std::vector<float>& alb = q->albedo;
    std::vector<float> p(np), r(nch);
    for (int k = 0; k < q->count; ++k) {
        const SeqFrame<1>* h = seq_header(q, k);
        const RadianceStage rs = {h->x, h->t_rem, h->t_low, h->t_high, h->in_range};
        for (int e = 0; e < np; ++e) p[e] = radiance_param(q->h_sky_params_ds.data(), np, e, rs, alb[e / kNbSkyParams]);
        for (int e = 0; e < nch; ++e) r[e] = radiance_param(q->h_sky_rad_ds.data(), nch, e, rs, alb[e]);
        unsigned char* rec = q->records.data() + (size_t)k * q->rec_bytes;
        FastChannel* fast = reinterpret_cast<FastChannel*>(rec + kSeqFrameHeader);
        SkyChannel* sky = reinterpret_cast<SkyChannel*>(rec + kSeqFrameHeader + (size_t)nch * sizeof(FastChannel));
        for (int c = 0; c < nch; ++c) fold_channel(&p[c * kNbSkyParams], r[c], q->variant, sky_scale, &sky[c], &fast[c]);
    }
}

// Headers from q->in_* (validated), then the channels: the one path of create and update, so an
// updated sequence's records are a new sequence's bits.  Throws before anything on the device
// or in q->records changes when a frame is refused.
void seq_restage(sunsky_sequence* q, const std::vector<float>& dirs, const std::vector<float>& turbidity,
                 const std::vector<float>& weights) {
    const std::vector<unsigned char> keep = q->records;
    q->records.assign((size_t)q->count * q->rec_bytes, 0);
    try {
        seq_fill_headers(q, dirs.data(), turbidity.data(), weights.data());
    } catch (...) {
        q->records = keep;
        throw;
    }
    if (q->device < 0) {
        seq_stage_host(q, q->kargs.sky_scale);
        return;
    }
    hip_check(hipMemcpy(q->d_frames.get(), q->records.data(), q->records.size(), hipMemcpyHostToDevice), "hipMemcpy");
    SeqStageArgs A;
    std::memset(&A, 0, sizeof(A));
    A.frames = q->d_frames.get();
    A.sky_params_ds = q->d_sky_params_ds;
    A.sky_rad_ds = q->d_sky_rad_ds;
    for (int c = 0; c < q->nch; ++c) A.albedo[c] = q->albedo[c];
    A.nch = q->nch;
    A.variant = q->variant;
    A.count = q->count;
    A.sky_scale = q->kargs.sky_scale;
    void* sargs[] = {&A};
    launch(q->mod, K_STAGE_SEQUENCE, (unsigned)std::min(q->count, 65535), kBlock, nullptr, sargs);
    hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    hip_check(hipMemcpy(q->records.data(), q->d_frames.get(), q->records.size(), hipMemcpyDeviceToHost), "hipMemcpy");
}

// ---- gradient records (sunsky_sequence_prepare_grad)
float* seq_grad_rec(sunsky_sequence* q, int k) {
    return reinterpret_cast<float*>(q->grads.data() + (size_t)k * seq_grad_bytes(q->nch));
}
const float* seq_grad_rec(const sunsky_sequence* q, int k) {
    return reinterpret_cast<const float*>(q->grads.data() + (size_t)k * seq_grad_bytes(q->nch));
}

// Frame k's staging scalars through tangent_stage_for (SunskyModel::tangent_stage's function)
// with the frame's local sun and turbidity.  s_k = |s| s^ enters the sequence normalised
// (seq_fill_headers), so the tangent of world axis a is the single emitter's along
// (I - s^ s^T) e_a / |s|: dlocal[a], deta[a].  Returns the frame's scalars with every tangent
// 0, from which the staging derives the turbidity and unit-elevation tangents.
TangentStage seq_grad_header(sunsky_sequence* q, int k) {
    const SeqFrame<1>* h = seq_header(q, k);
    const TangentFrame f = {q->to_local_d, h->sun_n, unit_angle_z(mk3(h->sun_n[0], h->sun_n[1], h->sun_n[2])),
                            h->turbidity, q->nch, q->albedo.data(), false};
    const double d[3] = {q->in_dirs[3 * (size_t)k], q->in_dirs[3 * (size_t)k + 1], q->in_dirs[3 * (size_t)k + 2]};
    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double u[3] = {d[0] / len, d[1] / len, d[2] / len};
    float* g = seq_grad_rec(q, k) + 2 * seq_grad_block(q->nch);
    for (int a = 0; a < 3; ++a) {
        float tangent[3];
        for (int r = 0; r < 3; ++r) tangent[r] = (float)(((r == a ? 1.0 : 0.0) - u[r] * u[a]) / len);
        const TangentStage s = tangent_stage_for(f, kJvpSunDirection, tangent, 3);
        for (int r = 0; r < 3; ++r) g[3 * a + r] = s.dsun_local[r];
        g[9 + a] = (float)s.deta;
    }
    const float zero = 0.f;
    return tangent_stage_for(f, kJvpTurbidity, &zero, 1);
}

// The gradient records of the current frames: headers on the host, the sky blocks by
// sunsky_stage_sequence_grad (host-only sequences: the same tangent_value on the host)
void seq_stage_grad(sunsky_sequence* q) {
    const int nch = q->nch, block = seq_grad_block(nch);
    q->grads.assign((size_t)q->count * seq_grad_bytes(nch), 0);
    std::vector<TangentStage> stages(q->count);
    for (int k = 0; k < q->count; ++k) stages[k] = seq_grad_header(q, k);
    if (q->device < 0) {
        for (int k = 0; k < q->count; ++k) {
            TangentStage st = stages[k], se = stages[k];
            st.dT = 1.0;
            se.dx = se.dx_per_eta;
            float* g = seq_grad_rec(q, k);
            for (int j = 0; j < nch * 10; ++j) {
                g[j] = tangent_value(q->h_sky_params_ds.data(), q->h_sky_rad_ds.data(), st, j);
                g[block + j] = tangent_value(q->h_sky_params_ds.data(), q->h_sky_rad_ds.data(), se, j);
            }
        }
        return;
    }
    hip_check(hipMemcpy(q->d_grads.get(), q->grads.data(), q->grads.size(), hipMemcpyHostToDevice), "hipMemcpy");
    hip_check(hipMemcpy(q->d_grad_stages.get(), stages.data(), sizeof(TangentStage) * stages.size(), hipMemcpyHostToDevice),
              "hipMemcpy");
    SeqGradStageArgs A = {q->d_grads.get(), q->d_grad_stages.get(), q->d_sky_params_ds, q->d_sky_rad_ds, nch, q->count};
    void* args[] = {&A};
    launch(q->mod, K_STAGE_SEQUENCE_GRAD, (unsigned)std::min(q->count, 65535), kBlock, nullptr, args);
    hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    hip_check(hipMemcpy(q->grads.data(), q->d_grads.get(), q->grads.size(), hipMemcpyDeviceToHost), "hipMemcpy");
}

// Workspace rows per workgroup of sunsky_sequence_eval_vjp: one while the waves' rows live in
// LDS (the workgroup adds them up), one per wave otherwise
size_t seq_grad_rows_per_block(const sunsky_sequence* q) {
    return q->count <= kSeqGradLdsFrames ? 1 : kBlock / 64;
}

// The grid of sunsky_sequence_eval_vjp over n rays: the kernel table's cap, then the
// workspace bound (rows of count x 5 floats)
unsigned seq_grad_grid(const sunsky_sequence* q, size_t n) {
    const size_t row = (size_t)q->count * kSeqGradSums * seq_grad_rows_per_block(q);
    const size_t cap = std::max<size_t>(1, kSeqGradWorkspaceFloats / row);
    return (unsigned)std::min<size_t>(grid_for(q->mod, K_SEQUENCE_EVAL_VJP_RGB, n), cap);
}

// ---- sampling tables (sunsky_sequence_prepare_sampling)
// sunsky_sequence_table / sunsky_sequence_suns on the host (host-only sequences): the same
// definitions through the SS_HD functions, with the host's libm
void seq_sampling_host(const sunsky_sequence* q, int nz, int nphi, std::vector<float>& f, std::vector<float>& B) {
    const SunskyKArgs& K = q->kargs;
    const bool rgb = q->variant == kRGB;
    const float cie = (float)kCieYNormalization;
    for (int i = 0; i < nz; ++i)
        for (int j = 0; j < nphi; ++j) {
            const float3_ wo = seq_cell_centre(nz, nphi, i, j);
            float acc[kNbWavelengths] = {0};
            for (int k = 0; k < q->count; ++k) {
                const SeqFrame<1>* h = seq_header(q, k);
                const SkyChannel* sky = seq_sky(q, k);
                const float gamma = unit_angle(mk3(h->sun_n[0], h->sun_n[1], h->sun_n[2]), wo);
                for (int c = 0; c < q->nch; ++c) {
                    const float v = K.sky_scale * render_sky(sky[c], wo.z, gamma);
                    acc[c] = fmaf(h->weight, rgb ? v * cie : v, acc[c]);
                }
            }
            float y = 0.f;
            if (rgb) y = luminance_rgb(acc);
            else {
                for (int c = 0; c < kNbWavelengths; ++c) y = fmaf(q->cie_y[c], acc[c], y);
                y = y / (float)kNbWavelengths;
            }
            f[(size_t)i * nphi + j] = std::fmax(y, 0.f);
        }
    const float* ds = q->h_sun_rad.data();
    for (int k = 0; k < q->count; ++k) {
        const SeqFrame<1>* h = seq_header(q, k);
        const float3_ sn = mk3(h->sun_n[0], h->sun_n[1], h->sun_n[2]);
        B[k] = 0.f;
        if (!(sn.z >= 0.f) || !(dot3(sn, sn) >= K.cos_cutoff)) continue;
        const RadianceStage rs = {0.f, h->t_rem, h->t_low, h->t_high, 1};
        int pos = 0;
        for (int j = 1; j < kNbSunSegments; ++j) pos += sn.z >= K.sun_seg_z[j] ? 1 : 0;
        const float frac = (float)pos / (float)kNbSunSegments;
        const float xs = (kHalfPi - acosf(sn.z)) - kHalfPi * (frac * frac * frac);
        const float cpsi = cos_psi(unit_angle(sn, sn), K.inv_sin2_half_ap);
        float y = 0.f;
        if (rgb) {
            constexpr int per_c = kNbSunCtrlPts * kNbSunLdParams;
            float v[3];
            for (int c = 0; c < 3; ++c) {
                float s[per_c];
                for (int e = 0; e < per_c; ++e) s[e] = sun_param(ds, q->sun_block, pos * (3 * per_c) + c * per_c + e, rs);
                v[c] = K.sun_scale * render_sun_rgb(s, 0, 0, xs, cpsi) * K.area_ratio * (float)kSpecToRgbSunConv;
            }
            y = luminance_rgb(v) * cie;
        } else {
            for (int c = 0; c < kNbWavelengths; ++c) {
                float sun = 0.f;
                for (int e = 0; e < kNbSunCtrlPts; ++e)
                    sun += powif_(xs, e) * sun_param(ds, q->sun_block, (pos * kNbWavelengths + c) * kNbSunCtrlPts + e, rs);
                const float ld = sun_limb_darkening(q->h_sun_ld.data(), c, c + 1, 0.f, cpsi);
                y = fmaf(q->cie_y[c], K.sun_scale * sun * ld * K.area_ratio, y);
            }
            y = y / (float)kNbWavelengths;
        }
        B[k] = std::fmax(y, 0.f);
    }
}

// Inclusive normalised CDF of n non-negative values: last entry 1, and 1 from the last
// non-zero value on, so a sample below 1 never lands on a trailing zero (all zero: uniform)
void seq_cdf(const double* v, int n, float* out) {
    double total = 0.0;
    int last = -1;
    for (int j = 0; j < n; ++j) {
        total += v[j];
        if (v[j] > 0.0) last = j;
    }
    double cum = 0.0;
    for (int j = 0; j < n; ++j) {
        cum += v[j];
        out[j] = last < 0 ? (float)((double)(j + 1) / (double)n) : (j >= last ? 1.f : (float)(cum / total));
    }
    out[n - 1] = 1.f;
}

// Floats of the device block: f, row_cdf, cell_cdf, frame_cdf, suns, each 16-byte aligned
struct SeqSamplingLayout {
    size_t f, row_cdf, cell_cdf, frame_cdf, suns, total;
    SeqSamplingLayout(int nz, int nphi, int count) {
        auto up = [](size_t x) { return (x + 3) & ~(size_t)3; };
        const size_t cells = (size_t)nz * (size_t)nphi;
        f = 0;
        row_cdf = up(cells);
        cell_cdf = row_cdf + up((size_t)nz);
        frame_cdf = cell_cdf + up(cells);
        suns = frame_cdf + up((size_t)count);
        total = suns + 4 * (size_t)count;
    }
};

// From the table and B_k to the distribution: masses, w_sky, q, the CDFs
void seq_sampling_finish(sunsky_sequence* q, int nz, int nphi, std::vector<float>&& f, std::vector<float>&& B) {
    const int K = q->count;
    const size_t cells = (size_t)nz * (size_t)nphi;
    std::vector<double> rows(nz), tmp(std::max(nphi, K));
    std::vector<float> row_cdf(nz), cell_cdf(cells), qv(K), frame_cdf(K);
    double S = 0.0;
    for (int i = 0; i < nz; ++i) {
        double r = 0.0;
        for (int j = 0; j < nphi; ++j) {
            tmp[j] = f[(size_t)i * nphi + j];
            r += tmp[j];
        }
        rows[i] = r;
        S += r;
        seq_cdf(tmp.data(), nphi, &cell_cdf[(size_t)i * nphi]);
    }
    seq_cdf(rows.data(), nz, row_cdf.data());
    const double omega = 2.0 * 3.14159265358979323846 / (double)cells;
    const double M = S * omega;
    double wb = 0.0;
    for (int k = 0; k < K; ++k) {
        tmp[k] = (double)seq_header(q, k)->weight * (double)B[k];
        wb += tmp[k];
    }
    const double P = 2.0 * 3.14159265358979323846 * (1.0 - (double)q->kargs.cos_cutoff) * wb;
    if (!std::isfinite(M + P) || !(M + P > 0.0))
        throw std::invalid_argument("the sequence is dark (every frame has zero weight or no radiance above the "
                                    "horizon): sky mass + sun mass == 0, there is nothing to sample");
    for (int k = 0; k < K; ++k) qv[k] = wb > 0.0 ? (float)(tmp[k] / wb) : 0.f;
    seq_cdf(tmp.data(), K, frame_cdf.data());
    const float w_sky = (float)(M / (M + P));
    q->samp_w_sky = w_sky;
    q->samp_sky_mass = (float)M;
    q->samp_sun_mass = (float)P;
    q->samp_f = std::move(f);
    q->samp_B = std::move(B);
    q->samp_row_cdf = std::move(row_cdf);
    q->samp_cell_cdf = std::move(cell_cdf);
    q->samp_q = std::move(qv);
    q->samp_frame_cdf = std::move(frame_cdf);
    for (int k = 0; k < K; ++k) seq_header(q, k)->pad[0] = q->samp_q[k];
    SeqSampling& s = q->samp;
    std::memset(&s, 0, sizeof(s));
    s.nz = nz;
    s.nphi = nphi;
    s.w_sky = w_sky;
    s.sky_coef = M > 0.0 ? (float)((double)w_sky / M) : 0.f;
    s.sun_coef = (1.f - w_sky) * q->kargs.sun_pdf;
    s.dphi = kTwoPi / (float)nphi;
    s.inv_dphi = (float)nphi / kTwoPi;
}

// ---- irradiance tables (sunsky_sequence_prepare_irradiance)
// sunsky_sequence_irradiance_table / _flux on the host (host-only sequences): the same
// definitions through the SS_HD functions, with the host's libm.  sky: [planes][nz][nphi],
// flux: [planes][count].
// The sky table over the frames [k0, k1) with their weights, or (unit) with weight 1: one frame's
// own table (sunsky_sequence_get_irradiance_frame_table) is the body run for that frame alone.
void seq_irradiance_sky_host(const sunsky_sequence* q, int nz, int nphi, const LambdaSet& L, int planes, int k0, int k1,
                             bool unit, float* sky_out) {
    const SunskyKArgs& K = q->kargs;
    const bool rgb = q->variant == kRGB;
    const float cie = (float)kCieYNormalization;
    const size_t cells = (size_t)nz * (size_t)nphi;
    for (int i = 0; i < nz; ++i)
        for (int j = 0; j < nphi; ++j) {
            const float3_ wo = seq_cell_centre(nz, nphi, i, j);
            float acc[kSeqIrrMaxPlanes] = {0};
            for (int k = k0; k < k1; ++k) {
                const SeqFrame<1>* h = seq_header(q, k);
                const SkyChannel* sky = seq_sky(q, k);
                const float w = unit ? 1.f : h->weight;
                const float gamma = unit_angle(mk3(h->sun_n[0], h->sun_n[1], h->sun_n[2]), wo);
                if (rgb) {
                    for (int c = 0; c < 3; ++c)
                        acc[c] = fmaf(w, K.sky_scale * render_sky(sky[c], wo.z, gamma) * cie, acc[c]);
                    continue;
                }
                for (int p = 0; p < planes; ++p) {
                    const int lo = L.lo[p], hi = lo + 1 < kNbWavelengths ? lo + 1 : lo;
                    const float f = L.f[p];
                    if (!(f >= 0.f)) continue;
                    float v = K.sky_scale * render_sky(sky[lo], wo.z, gamma);
                    if (f != 0.f) v = lerpf_(v, K.sky_scale * render_sky(sky[hi], wo.z, gamma), f);
                    acc[p] = fmaf(w, v, acc[p]);
                }
            }
            for (int p = 0; p < planes; ++p) sky_out[(size_t)p * cells + (size_t)i * nphi + j] = acc[p];
        }
}

void seq_irradiance_host(const sunsky_sequence* q, int nz, int nphi, const LambdaSet& L, int planes, float s2,
                         std::vector<float>& sky_out, std::vector<float>& flux) {
    const SunskyKArgs& K = q->kargs;
    const bool rgb = q->variant == kRGB;
    const float cie = (float)kCieYNormalization;
    seq_irradiance_sky_host(q, nz, nphi, L, planes, 0, q->count, false, sky_out.data());
    const float* ds = q->h_sun_rad.data();
    const float ring = kTwoPi / (float)kSeqFluxNphi;
    constexpr int kPoints = kSeqFluxNu * kSeqFluxNphi;
    std::vector<float> term((size_t)planes * kPoints);
    for (int k = 0; k < q->count; ++k) {
        const SeqFrame<1>* h = seq_header(q, k);
        const float3_ sn = mk3(h->sun_n[0], h->sun_n[1], h->sun_n[2]);
        const RadianceStage rs = {0.f, h->t_rem, h->t_low, h->t_high, 1};
        float3_ fs, ft;
        coordinate_system(sn, &fs, &ft);
        std::fill(term.begin(), term.end(), 0.f);
        for (int lane = 0; lane < kPoints; ++lane) {
            const SeqFluxPoint pt = seq_flux_point(s2, lane / kSeqFluxNphi, lane % kSeqFluxNphi);
            const float3_ d = frame_to_world(fs, ft, sn, mk3(pt.x, pt.y, pt.z));
            if (!(sn.z >= 0.f && d.z >= 0.f)) continue;
            const float ct = std::fmin(d.z, 1.f);
            int pos = 0;
            for (int j = 1; j < kNbSunSegments; ++j) pos += ct >= K.sun_seg_z[j] ? 1 : 0;
            const float frac = (float)pos / (float)kNbSunSegments;
            const float xs = (kHalfPi - acosf(ct)) - kHalfPi * (frac * frac * frac);
            if (rgb) {
                constexpr int per_c = kNbSunCtrlPts * kNbSunLdParams;
                for (int c = 0; c < 3; ++c) {
                    float s[per_c];
                    for (int e = 0; e < per_c; ++e) s[e] = sun_param(ds, q->sun_block, pos * (3 * per_c) + c * per_c + e, rs);
                    const float v = K.sun_scale * render_sun_rgb(s, 0, 0, xs, pt.u) * K.area_ratio * (float)kSpecToRgbSunConv;
                    term[(size_t)c * kPoints + lane] = pt.W * (v * cie);
                }
                continue;
            }
            for (int p = 0; p < planes; ++p) {
                const int lo = L.lo[p], hi = lo + 1;
                const float f = L.f[p];
                if (!(f >= 0.f)) continue;
                auto poly = [&](int c) {
                    float res = 0.f;
                    for (int e = 0; e < kNbSunCtrlPts; ++e)
                        res += powif_(xs, e) * sun_param(ds, q->sun_block, (pos * kNbWavelengths + c) * kNbSunCtrlPts + e, rs);
                    return res;
                };
                float sun = poly(lo);
                if (f != 0.f) sun = lerpf_(sun, hi < kNbWavelengths ? poly(hi) : 0.f, f);
                const float ld = sun_limb_darkening(q->h_sun_ld.data(), lo, hi, f, pt.u);
                term[(size_t)p * kPoints + lane] = pt.W * (K.sun_scale * sun * ld * K.area_ratio);
            }
        }
        for (int p = 0; p < planes; ++p) {   // wave_sum's tree: lane l += lane l + off, off = 32 .. 1
            float* t = &term[(size_t)p * kPoints];
            for (int off = kPoints / 2; off > 0; off >>= 1)
                for (int l = 0; l < off; ++l) t[l] += t[l + off];
            flux[(size_t)p * q->count + k] = ring * t[0];
        }
    }
}

// The image the hot path walks, from the tables: per cell c_ij.xyz and omega R_p[i, j], then per
// frame with a non-zero w_k F_k (order kept) s_k.xyz and w_k F_k[p]; records of seq_irr_record
// floats.  Returns the number of sun records; kept: their frames.
int seq_irradiance_image(const sunsky_sequence* q, int nz, int nphi, int planes, float omega, const std::vector<float>& sky,
                         const std::vector<float>& flux, std::vector<float>& image, std::vector<int>& kept) {
    const int rec = seq_irr_record(planes);
    const size_t cells = (size_t)nz * (size_t)nphi;
    image.assign((cells + (size_t)q->count) * rec, 0.f);
    for (int i = 0; i < nz; ++i)
        for (int j = 0; j < nphi; ++j) {
            const size_t cell = (size_t)i * nphi + j;
            const float3_ c = seq_cell_centre(nz, nphi, i, j);
            float* r = &image[cell * rec];
            r[0] = c.x; r[1] = c.y; r[2] = c.z;
            for (int p = 0; p < planes; ++p) r[3 + p] = omega * sky[(size_t)p * cells + cell];
        }
    int nsuns = 0;
    for (int k = 0; k < q->count; ++k) {
        const SeqFrame<1>* h = seq_header(q, k);
        float* r = &image[(cells + (size_t)nsuns) * rec];
        bool any = false;
        for (int p = 0; p < planes; ++p) {
            r[3 + p] = h->weight * flux[(size_t)p * q->count + k];
            any = any || r[3 + p] != 0.f;
        }
        if (!any) continue;
        r[0] = h->sun_n[0]; r[1] = h->sun_n[1]; r[2] = h->sun_n[2];
        kept.push_back(k);
        ++nsuns;
    }
    image.resize((cells + (size_t)nsuns) * rec);
    return nsuns;
}

// The grid column of every frame's sun (sunsky_sequence_get_irradiance_sun_columns): the column
// seq_sky_cell takes for a direction, with the host's atan2f.  A sun at the pole: column 0.
std::vector<int> seq_irradiance_sun_columns(const sunsky_sequence* q, int nphi) {
    std::vector<int> cols((size_t)q->count);
    const float inv_dphi = (float)nphi / kTwoPi;
    for (int k = 0; k < q->count; ++k) {
        const SeqFrame<1>* h = seq_header(q, k);
        float phi = atan2f(h->sun_n[1], h->sun_n[0]);
        phi = phi < 0.f ? phi + kTwoPi : phi;
        cols[(size_t)k] = std::min(std::max((int)(phi * inv_dphi), 0), nphi - 1);
    }
    return cols;
}

// The workspace bound of the irradiance gradients in floats: kSeqIrrGradWorkspaceFloats, or the
// smaller value SUNSKY_AMD_IRRADIANCE_GRAD_WORKSPACE_FLOATS gives (read at every prepare).
size_t seq_irr_grad_cap() {
    size_t cap = kSeqIrrGradWorkspaceFloats;
    if (const char* e = std::getenv("SUNSKY_AMD_IRRADIANCE_GRAD_WORKSPACE_FLOATS")) {
        const long long v = std::atoll(e);
        if (v >= 1 && (unsigned long long)v < cap) cap = (size_t)v;
    }
    return cap;
}

// What sunsky_sequence_irradiance_vjp reads beside the forward's image, for the tables as they
// are now: every frame's local sun direction, the unweighted fluxes, every frame's sun column
// (sunsky_sequence_irradiance_horizon_vjp's sectors) and the workspace of the most slices the
// bound allows.  A host-only sequence only changes state.
void seq_stage_irradiance_grad(sunsky_sequence* q) {
    q->irr_grad_ready = false;
    if (q->device >= 0) {
        q->d_irr_grad.reset();
        const int planes = q->irr_planes, count = q->count;
        const size_t cells = (size_t)q->irr_nz * (size_t)q->irr_nphi, entries = cells + (size_t)count;
        q->irr_grad_cap = seq_irr_grad_cap();
        const size_t slices = seq_irr_grad_max_slices(planes, cells, count, q->irr_grad_cap);
        static_assert(sizeof(int) == sizeof(float), "the suns' columns lie between the fluxes and the workspace");
        const size_t cols_at = 4 * (size_t)count + (size_t)planes * count, head = cols_at + (size_t)count;
        std::vector<float> h(head, 0.f);
        for (int k = 0; k < count; ++k) {
            const SeqFrame<1>* f = seq_header(q, k);
            for (int a = 0; a < 3; ++a) h[4 * (size_t)k + a] = f->sun_n[a];
        }
        std::copy(q->irr_flux.begin(), q->irr_flux.end(), h.begin() + 4 * (size_t)count);
        std::memcpy(h.data() + cols_at, q->irr_sun_cols.data(), sizeof(int) * (size_t)count);
        q->d_irr_grad.alloc(head + slices * planes * entries);
        hip_check(hipMemcpy(q->d_irr_grad.get(), h.data(), sizeof(float) * head, hipMemcpyHostToDevice), "hipMemcpy");
        SeqIrrGrad& g = q->irr_grad;
        std::memset(&g, 0, sizeof(g));
        g.suns = q->d_irr_grad.get();
        g.flux = q->d_irr_grad.get() + 4 * (size_t)count;
        g.rows = q->d_irr_grad.get() + head;
        q->d_irr_grad_cols = reinterpret_cast<const int*>(q->d_irr_grad.get() + cols_at);
        g.omega = q->irr_omega;
        g.count = count;
    }
    q->irr_grad_ready = true;
}

// The cap of the series' K * P * n_z * n_phi in floats: kSeqIrrSeriesMaxFloats, or the smaller
// value SUNSKY_AMD_IRRADIANCE_SERIES_MAX_FLOATS gives (read at every prepare).
size_t seq_irr_series_cap() {
    size_t cap = kSeqIrrSeriesMaxFloats;
    if (const char* e = std::getenv("SUNSKY_AMD_IRRADIANCE_SERIES_MAX_FLOATS")) {
        const long long v = std::atoll(e);
        if (v >= 1 && (unsigned long long)v < cap) cap = (size_t)v;
    }
    return cap;
}

// sunsky_sequence_irradiance_series_table over `groups` groups of `group` frames from frame0:
// into the groups' images, or (raw) one frame's plain table.  The caller synchronises.
void seq_irr_series_table(const sunsky_sequence* q, float* image, float* raw, int group, int groups, int frame0) {
    SeqIrrSeriesTableArgs T;
    std::memset(&T, 0, sizeof(T));
    T.image = image;
    T.raw = raw;
    T.cells = q->irr.cells;
    T.cells_rec = seq_irr_record(q->irr_planes);
    T.L = q->irr_L;
    T.nz = q->irr_nz;
    T.nphi = q->irr_nphi;
    T.planes = q->irr_planes;
    T.group = group;
    T.groups = groups;
    T.rec = seq_irr_record(group * q->irr_planes);
    T.frame0 = frame0;
    T.omega = q->irr_omega;
    const SunskyKArgs* K = q->d_state.get();
    SeqArgs A = q->args();
    void* args[] = {&K, &A, &T};
    const size_t lanes = (size_t)q->irr_nz * (size_t)q->irr_nphi * (size_t)groups;
    launch(q->mod, K_SEQUENCE_IRRADIANCE_SERIES_TABLE,
           grid_for(q->mod, K_SEQUENCE_IRRADIANCE_SERIES_TABLE, lanes, /*tunable=*/false), kBlock, nullptr, args);
}

// What sunsky_sequence_irradiance_series walks, for the tables as they are now: every group's
// image written on the device, then per value its frame's sun record and column.  Refuses above
// the cap (`quiet`: leaves the series unprepared instead); a host-only sequence only changes state.
void seq_stage_irradiance_series(sunsky_sequence* q, bool quiet = false) {
    q->irr_series_ready = false;
    const int planes = q->irr_planes, count = q->count;
    const size_t cells = (size_t)q->irr_nz * (size_t)q->irr_nphi, cap = seq_irr_series_cap();
    if ((size_t)count * (size_t)planes * cells > cap) {
        if (quiet) return;
        throw std::invalid_argument("the irradiance series of " + std::to_string(count) + " frames x " + std::to_string(planes) +
                                    " planes x " + std::to_string(cells) + " cells exceeds the cap of " + std::to_string(cap) +
                                    " floats (2^26, lowered by SUNSKY_AMD_IRRADIANCE_SERIES_MAX_FLOATS)");
    }
    if (q->device >= 0) {
        q->d_irr_series.reset();
        const int G = seq_irr_series_group(planes), values = G * planes, rec = seq_irr_record(values);
        const int groups = (count + G - 1) / G;
        const size_t image = cells * (size_t)rec, images = image * (size_t)groups, nvalues = (size_t)groups * values;
        static_assert(sizeof(int) == sizeof(float), "the values' columns lie behind their sun records");
        q->d_irr_series.alloc(images + 5 * nvalues);
        float* const d = q->d_irr_series.get();
        hip_check(hipMemset(d, 0, sizeof(float) * images), "hipMemset");
        seq_irr_series_table(q, d, nullptr, G, groups, 0);
        std::vector<float> suns(5 * nvalues, 0.f);   // {s_k.xyz, F_k[p]} per value, then the columns
        int* const cols = reinterpret_cast<int*>(suns.data() + 4 * nvalues);
        for (int k = 0; k < count; ++k) {
            const SeqFrame<1>* h = seq_header(q, k);
            for (int p = 0; p < planes; ++p) {
                const size_t v = (size_t)k * planes + p;   // group k / G, value (k % G) * planes + p
                float* r = &suns[4 * v];
                r[0] = h->sun_n[0]; r[1] = h->sun_n[1]; r[2] = h->sun_n[2];
                r[3] = q->irr_flux[(size_t)p * count + k];
                cols[v] = q->irr_sun_cols[(size_t)k];
            }
        }
        hip_check(hipMemcpy(d + images, suns.data(), sizeof(float) * suns.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
        SeqIrrSeries& s = q->irr_series;
        std::memset(&s, 0, sizeof(s));
        s.images = d;
        s.suns = d + images;
        s.sun_cols = reinterpret_cast<const int*>(d + images + 4 * nvalues);
        s.image_floats = image;
        s.nz = q->irr_nz;
        s.nphi = q->irr_nphi;
        s.values = values;
        s.rec = rec;
        q->irr_series_groups = groups;
    }
    q->irr_series_ready = true;
}

}  // namespace

extern "C" {

int sunsky_sequence_create(const sunsky_emitter* e, int count, const float* sun_dirs, const float* turbidity,
                           const float* weights, sunsky_sequence** out) {
    SUNSKY_PHASE("InitScene", "sequence_create");
    if (!e || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter / output pointer");
    *out = nullptr;
    if (count < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "a sequence needs at least one frame (count >= 1)");
    if (!sun_dirs) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sun direction array");
    return guarded([&] {
        std::unique_ptr<sunsky_sequence> q(new sunsky_sequence());
        const EmitterSnapshot em = emitter_snapshot(e);
        const SunskyModel& model = em.model;
        q->kargs = em.kargs;
        q->kargs.sun_table = nullptr;   // no per-frame sun table: the disc lanes lerp the raw dataset
        q->kargs.sun_ld = nullptr;
        q->count = count;
        q->nch = model.nch();
        q->variant = model.variant();
        q->precision = em.precision;
        q->sun_block = q->variant == kSpectral ? kSunSpecTableSize : kSunRgbTableSize;
        q->rec_bytes = kSeqFrameHeader + (size_t)q->nch * (sizeof(FastChannel) + sizeof(SkyChannel));
        std::memcpy(q->cie_y, model.cie_y(), sizeof(q->cie_y));
        // the frames as given, defaults resolved: what sunsky_sequence_update keeps for a NULL array
        std::vector<float> dirs(sun_dirs, sun_dirs + 3 * (size_t)count);
        std::vector<float> T(count, model.turbidity()), w(count, 1.f);
        if (turbidity) T.assign(turbidity, turbidity + count);
        if (weights) w.assign(weights, weights + count);
        q->albedo = model.albedo();
        std::memcpy(q->to_local_d, model.to_local_d(), sizeof(q->to_local_d));
        if (em.device < 0) {
            q->h_sun_rad = model.sun_rad_ds();   // prepare_sampling's disc term on the host
            q->h_sun_ld = model.sun_ld();
            q->h_sky_params_ds = model.sky_params_ds();
            q->h_sky_rad_ds = model.sky_rad_ds();
            seq_restage(q.get(), dirs, T, w);
            q->in_dirs = std::move(dirs); q->in_turbidity = std::move(T); q->in_weights = std::move(w);
            *out = q.release();
            return;
        }
        DeviceScope g(em.device);
        q->mod = em.mod;
        q->device = em.device;   // from here on the destructor drains the device before the owners free
        const std::vector<float>& su = model.sun_rad_ds();
        const std::vector<float>& ld = model.sun_ld();
        const std::vector<float>& sp = model.sky_params_ds();
        const std::vector<float>& sr = model.sky_rad_ds();
        q->d_frames.alloc((size_t)count * q->rec_bytes);
        q->d_sun_rad.alloc(su.size());
        q->d_sun_ld.alloc(kNbWavelengths * kNbSunLdParams);
        q->d_state.alloc(1);
        q->d_sky_ds.alloc(sp.size() + sr.size());
        hip_check(hipMemcpy(q->d_sun_rad.get(), su.data(), sizeof(float) * su.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemset(q->d_sun_ld.get(), 0, sizeof(float) * q->d_sun_ld.size()), "hipMemset");
        hip_check(hipMemcpy(q->d_sun_ld.get(), ld.data(), sizeof(float) * std::min<size_t>(ld.size(), q->d_sun_ld.size()),
                            hipMemcpyHostToDevice), "hipMemcpy");
        // the raw sky datasets, the sequence's own copy: update restages from it when the parent is gone
        hip_check(hipMemcpy(q->d_sky_ds.get(), sp.data(), sizeof(float) * sp.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(q->d_sky_ds.get() + sp.size(), sr.data(), sizeof(float) * sr.size(), hipMemcpyHostToDevice), "hipMemcpy");
        q->d_sky_params_ds = q->d_sky_ds.get();
        q->d_sky_rad_ds = q->d_sky_ds.get() + sp.size();
        q->kargs.sun_ld = q->d_sun_ld.get();
        hip_check(hipMemcpy(q->d_state.get(), &q->kargs, sizeof(SunskyKArgs), hipMemcpyHostToDevice), "hipMemcpy");
        seq_restage(q.get(), dirs, T, w);
        q->in_dirs = std::move(dirs); q->in_turbidity = std::move(T); q->in_weights = std::move(w);
        *out = q.release();
    });
}

int sunsky_sequence_update(sunsky_sequence* seq, const float* sun_dirs, const float* turbidity, const float* weights) {
    SUNSKY_PHASE("InitScene", "sequence_update");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        const size_t K = (size_t)seq->count;
        std::vector<float> dirs = seq->in_dirs, T = seq->in_turbidity, w = seq->in_weights;
        if (sun_dirs) dirs.assign(sun_dirs, sun_dirs + 3 * K);
        if (turbidity) T.assign(turbidity, turbidity + K);
        if (weights) w.assign(weights, weights + K);
        DeviceScope g(seq->device);   // host-only (-1): no device to scope
        // nothing may still read the old records
        if (seq->device >= 0) hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        seq_restage(seq, dirs, T, w);   // throws with the sequence untouched when a frame is refused
        seq->in_dirs = std::move(dirs); seq->in_turbidity = std::move(T); seq->in_weights = std::move(w);
        // the sampling distribution described the old frames
        seq->samp_nz = seq->samp_nphi = 0;
        seq->irr_nz = seq->irr_nphi = seq->irr_planes = 0;   // and so did the irradiance tables
        seq->irr_grad_ready = false;                         // and what their gradients read (wanted stays)
        seq->irr_series_ready = false;                       // and the per-frame series (wanted stays)
        if (seq->grad_ready) seq_stage_grad(seq);
    });
}

int sunsky_sequence_prepare_grad(sunsky_sequence* seq) {
    SUNSKY_PHASE("InitScene", "sequence_prepare_grad");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        DeviceScope g(seq->device);   // host-only (-1): no device to scope
        if (seq->device >= 0) {
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // nothing may still read the old records
            if (!seq->d_grad_rows.get()) {   // once: the records, the staging scalars, the rows of the largest grid
                seq->grad_max_grid = seq_grad_grid(seq, ~(size_t)0 / 2);
                const size_t rows = (size_t)seq->grad_max_grid * seq_grad_rows_per_block(seq);
                if (!seq->d_grads.get()) seq->d_grads.alloc((size_t)seq->count * seq_grad_bytes(seq->nch));
                if (!seq->d_grad_stages.get()) seq->d_grad_stages.alloc((size_t)seq->count);
                seq->d_grad_rows.alloc(rows * (size_t)seq->count * kSeqGradSums);
            }
        }
        seq_stage_grad(seq);
        seq->grad_ready = true;
    });
}

int sunsky_sequence_get_frame_tangent(const sunsky_sequence* seq, int k, float* dsky_turbidity, float* dsky_elevation,
                                      float dsun_local[9], float deta[3]) {
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (k < 0 || k >= seq->count) return fail(SUNSKY_ERROR_INVALID_VALUE, "frame index out of range");
    return guarded([&] {
        seq->require_grad();
        const int block = seq_grad_block(seq->nch);
        const float* g = seq_grad_rec(seq, k);
        const size_t sky = sizeof(float) * (size_t)seq->nch * 10;
        if (dsky_turbidity) std::memcpy(dsky_turbidity, g, sky);
        if (dsky_elevation) std::memcpy(dsky_elevation, g + block, sky);
        if (dsun_local) std::memcpy(dsun_local, g + 2 * block, 9 * sizeof(float));
        if (deta) std::memcpy(deta, g + 2 * block + 9, 3 * sizeof(float));
    });
}

int sunsky_sequence_eval_vjp(const sunsky_sequence* seq, sunsky_vec3_in wi, const float* lam_host, int m,
                             const uint8_t* active, size_t n, const float* d_out, size_t ostride, float* grad_weight,
                             float* grad_turbidity, float* grad_sun_dir, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_eval_vjp");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    const bool spec = seq->variant == kSpectral;
    if (int rc = check_sequence_lambda(spec, lam_host, m)) return rc;
    if (n == 0) return SUNSKY_OK;
    if (!wi.x || !wi.y || !wi.z) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray pointer");
    if (!d_out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null cotangent (d_out)");
    if ((spec ? m : 3) > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    return guarded([&] {
        seq->require_grad();   // first: the message names the missing call on any sequence
        Launcher lc(seq, stream);
        if (!grad_weight && !grad_turbidity && !grad_sun_dir) return;
        const unsigned grid = seq_grad_grid(seq, n);   // <= grad_max_grid: the workspace holds its rows
        const bool lds = seq->count <= kSeqGradLdsFrames;
        SeqArgs A = seq->args();
        SeqGradArgs G = {seq->d_grads.get(), d_out, ostride, seq->d_grad_rows.get(), lds ? 1 : 0, 0};
        const unsigned dyn = lds ? (unsigned)(sizeof(float) * (kBlock / 64) * (size_t)seq->count * kSeqGradSums) : 0u;
        // reference arithmetic whatever the sequence's precision: both names run the same body
        if (!spec) {
            void* args[] = {&lc.K, &A, &G, (void*)&wi.x, (void*)&wi.y, (void*)&wi.z, &active, &n};
            lc.launch(K_SEQUENCE_EVAL_VJP_RGB, grid, kBlock, args, dyn, SUNSKY_PRECISION_REFERENCE);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&lc.K, &A, &G, &L, (void*)&wi.x, (void*)&wi.y, (void*)&wi.z, &active, &n};
            lc.launch(K_SEQUENCE_EVAL_VJP_SPEC, grid, kBlock, args, dyn, SUNSKY_PRECISION_REFERENCE);
        }
        const float* rows = seq->d_grad_rows.get();
        unsigned nrows = grid * (unsigned)seq_grad_rows_per_block(seq);
        int count = seq->count;
        void* rargs[] = {(void*)&rows, &nrows, &count, &grad_weight, &grad_turbidity, &grad_sun_dir};
        lc.launch(K_SEQUENCE_GRAD_REDUCE, (unsigned)std::min(count, 65535), kSeqGradReduceBlock, rargs);
    });
}

void sunsky_sequence_destroy(sunsky_sequence* seq) { delete seq; }

int sunsky_sequence_info(const sunsky_sequence* seq, sunsky_sequence_desc* out) {
    if (!seq || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    out->count = seq->count;
    out->variant = seq->variant;
    out->nb_channels = seq->nch;
    out->precision = seq->precision;
    out->device = seq->device;
    return SUNSKY_OK;
}

int sunsky_sequence_set_precision(sunsky_sequence* seq, int precision) {
    if (!seq || (precision != SUNSKY_PRECISION_FAST && precision != SUNSKY_PRECISION_REFERENCE))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "invalid precision mode");
    seq->precision = precision;
    return SUNSKY_OK;
}

int sunsky_sequence_get_frame(const sunsky_sequence* seq, int k, float sun_dir_local[3], float* weight, float* turbidity,
                              float* sky_params, float* sky_radiance) {
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (k < 0 || k >= seq->count) return fail(SUNSKY_ERROR_INVALID_VALUE, "frame index out of range");
    const SeqFrame<1>* h = seq_header(seq, k);
    const SkyChannel* sky = seq_sky(seq, k);
    if (sun_dir_local) std::memcpy(sun_dir_local, h->sun_n, 3 * sizeof(float));
    if (weight) *weight = h->weight;
    if (turbidity) *turbidity = h->turbidity;
    for (int c = 0; c < seq->nch; ++c) {
        const SkyChannel& ch = sky[c];
        const float p[kNbSkyParams] = {ch.A, ch.B, ch.C, ch.D, ch.E, ch.F, ch.G, ch.H, ch.I};
        if (sky_params) std::memcpy(sky_params + (size_t)c * kNbSkyParams, p, sizeof(p));
        if (sky_radiance) sky_radiance[c] = ch.rad;
    }
    return SUNSKY_OK;
}

int sunsky_sequence_eval(const sunsky_sequence* seq, sunsky_vec3_in w, const float* lam_host, int m,
                         const uint8_t* active, size_t n, float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_eval");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    const bool spec = seq->variant == kSpectral;
    if (int rc = check_sequence_lambda(spec, lam_host, m)) return rc;
    if (n == 0) return SUNSKY_OK;
    if (!w.x || !w.y || !w.z || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / output pointer");
    if ((spec ? m : 3) > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    return guarded([&] {
        Launcher lc(seq, stream);
        SeqArgs A = seq->args();
        if (!spec) {
            void* args[] = {&lc.K, &A, (void*)&w.x, (void*)&w.y, (void*)&w.z, &active, &n, &out, &ostride};
            lc.run(K_SEQUENCE_EVAL_RGB, n, args);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&lc.K, &A, &L, (void*)&w.x, (void*)&w.y, (void*)&w.z, &active, &n, &out, &ostride};
            lc.run(K_SEQUENCE_EVAL_SPEC, n, args);
        }
    });
}

int sunsky_sequence_bake_latlong(const sunsky_sequence* seq, int width, int height, float theta0, float theta1,
                                 float phi0, float phi1, const float* lam_host, int m, float* out, size_t ostride,
                                 void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_bake_latlong");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    const bool spec = seq->variant == kSpectral;
    LatLong G;
    if (int rc = check_bake(spec, width, height, theta0, theta1, phi0, phi1, lam_host, m, out, ostride, &G)) return rc;
    const size_t n = (size_t)width * (size_t)height;
    return guarded([&] {
        Launcher lc(seq, stream);
        // the angle tables are per sequence, ordered between bakes as sunsky_bake_latlong's
        float* tab = seq->bake.begin(lc.s, 2 * (size_t)width + 2 * (size_t)height);
        G.tab = tab;
        {
            void* targs[] = {&G, &tab};
            lc.launch(K_LATLONG_TABLES, (unsigned)((std::max(width, height) + kBlock - 1) / kBlock), kBlock, targs);
        }
        SeqArgs A = seq->args();
        if (!spec) {
            void* args[] = {&lc.K, &A, &G, &out, &ostride};
            lc.run(K_SEQUENCE_BAKE_RGB, n, args);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&lc.K, &A, &G, &L, &out, &ostride};
            lc.run(K_SEQUENCE_BAKE_SPEC, n, args);
        }
        seq->bake.end(lc.s);
    });
}

int sunsky_sequence_prepare_sampling(sunsky_sequence* seq, int n_z, int n_phi) {
    SUNSKY_PHASE("InitScene", "sequence_prepare_sampling");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (n_z < 1 || n_z > kSeqSampleMaxZ || n_phi < 4 || n_phi > kSeqSampleMaxPhi ||
        (int64_t)n_z * n_phi > kSeqSampleMaxCells)
        return fail(SUNSKY_ERROR_INVALID_VALUE,
                    "sampling table size out of range: 1 <= n_z <= 1024, 4 <= n_phi <= 4096, n_z * n_phi <= 2^20");
    return guarded([&] {
        const size_t cells = (size_t)n_z * (size_t)n_phi;
        std::vector<float> f(cells), B(seq->count);
        if (seq->device < 0) {
            seq_sampling_host(seq, n_z, n_phi, f, B);
            seq_sampling_finish(seq, n_z, n_phi, std::move(f), std::move(B));
            seq->samp_nz = n_z;
            seq->samp_nphi = n_phi;
            return;
        }
        DeviceScope g(seq->device);
        const SeqSamplingLayout lay(n_z, n_phi, seq->count);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // nothing may still read the old tables
        seq->samp_nz = seq->samp_nphi = 0;
        seq->d_samp.alloc(lay.total);   // frees the old tables first
        float* const samp = seq->d_samp.get();
        hip_check(hipMemset(samp, 0, sizeof(float) * lay.total), "hipMemset");
        SeqTableArgs T;
        std::memset(&T, 0, sizeof(T));
        T.f = samp + lay.f;
        T.B = samp + lay.suns;   // B_k rests where the sun records go
        std::memcpy(T.cie_y, seq->cie_y, sizeof(T.cie_y));
        T.nz = n_z;
        T.nphi = n_phi;
        const SunskyKArgs* K = seq->d_state.get();
        SeqArgs A = seq->args();
        void* args[] = {&K, &A, &T};
        launch(seq->mod, K_SEQUENCE_TABLE, grid_for(seq->mod, K_SEQUENCE_TABLE, cells, /*tunable=*/false), kBlock, nullptr, args);
        launch(seq->mod, K_SEQUENCE_SUNS, (unsigned)std::min(seq->count, 65535), kWaveBlock, nullptr, args);
        hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
        hip_check(hipMemcpy(f.data(), T.f, sizeof(float) * cells, hipMemcpyDeviceToHost), "hipMemcpy");
        hip_check(hipMemcpy(B.data(), T.B, sizeof(float) * seq->count, hipMemcpyDeviceToHost), "hipMemcpy");
        seq_sampling_finish(seq, n_z, n_phi, std::move(f), std::move(B));
        std::vector<float> block(lay.total, 0.f);
        std::copy(seq->samp_f.begin(), seq->samp_f.end(), block.begin() + lay.f);
        std::copy(seq->samp_row_cdf.begin(), seq->samp_row_cdf.end(), block.begin() + lay.row_cdf);
        std::copy(seq->samp_cell_cdf.begin(), seq->samp_cell_cdf.end(), block.begin() + lay.cell_cdf);
        std::copy(seq->samp_frame_cdf.begin(), seq->samp_frame_cdf.end(), block.begin() + lay.frame_cdf);
        for (int k = 0; k < seq->count; ++k) {
            const SeqFrame<1>* h = seq_header(seq, k);
            float* r = &block[lay.suns + 4 * (size_t)k];
            r[0] = h->sun_n[0]; r[1] = h->sun_n[1]; r[2] = h->sun_n[2];
            r[3] = seq->samp_q[k];
        }
        hip_check(hipMemcpy(samp, block.data(), sizeof(float) * lay.total, hipMemcpyHostToDevice), "hipMemcpy");
        // q_k into the records (SeqFrame::pad[0]): the sample kernels read it beside the header
        hip_check(hipMemcpy(seq->d_frames.get(), seq->records.data(), seq->records.size(), hipMemcpyHostToDevice), "hipMemcpy");
        SeqSampling& s = seq->samp;
        s.f = samp + lay.f;
        s.row_cdf = samp + lay.row_cdf;
        s.cell_cdf = samp + lay.cell_cdf;
        s.frame_cdf = samp + lay.frame_cdf;
        s.suns = samp + lay.suns;
        seq->samp_nz = n_z;
        seq->samp_nphi = n_phi;
    });
}

int sunsky_sequence_sampling_info(const sunsky_sequence* seq, sunsky_sequence_sampling_desc* out) {
    if (!seq || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    return guarded([&] {
        seq->require_sampling();
        out->n_z = seq->samp_nz;
        out->n_phi = seq->samp_nphi;
        out->w_sky = seq->samp_w_sky;
        out->sky_mass = seq->samp_sky_mass;
        out->sun_mass = seq->samp_sun_mass;
    });
}

int sunsky_sequence_get_sampling_table(const sunsky_sequence* seq, int id, float* out, size_t cap, size_t* count) {
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        seq->require_sampling();
        const std::vector<float>* t = nullptr;
        switch (id) {
            case SUNSKY_SEQUENCE_TABLE_SKY: t = &seq->samp_f; break;
            case SUNSKY_SEQUENCE_TABLE_ROW_CDF: t = &seq->samp_row_cdf; break;
            case SUNSKY_SEQUENCE_TABLE_CELL_CDF: t = &seq->samp_cell_cdf; break;
            case SUNSKY_SEQUENCE_TABLE_Q: t = &seq->samp_q; break;
            case SUNSKY_SEQUENCE_TABLE_FRAME_CDF: t = &seq->samp_frame_cdf; break;
            case SUNSKY_SEQUENCE_TABLE_B: t = &seq->samp_B; break;
            default: throw std::invalid_argument("unknown sequence sampling table id");
        }
        if (count) *count = t->size();
        if (out) std::memcpy(out, t->data(), sizeof(float) * std::min(cap, t->size()));
    });
}

int sunsky_sequence_sample_direction(const sunsky_sequence* seq, const float* ux, const float* uy, sunsky_vec3_in it_p,
                                     const float* lam_host, int m, const uint8_t* active, size_t n,
                                     sunsky_vec3_out ds_d, float* ds_pdf, float* ds_dist, sunsky_vec3_out ds_p,
                                     float* weight, size_t wstride, void* stream) {
    SUNSKY_PHASE("EndpointSampleDirection", "sequence_sample_direction");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    const bool spec = seq->variant == kSpectral;
    if (int rc = check_sequence_lambda(spec, lam_host, m)) return rc;
    if (n == 0) return SUNSKY_OK;
    if (!ux || !uy || !ds_d.x || !ds_d.y || !ds_d.z || !ds_pdf || !weight)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null sample / output pointer");
    if ((spec ? m : 3) > 1 && wstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "weight_stride < n");
    if (int rc = check_optional_vec3(it_p, "it_p")) return rc;
    if (int rc = check_optional_vec3(ds_p, "ds_p")) return rc;
    return guarded([&] {
        seq->require_sampling();   // first: the message names the missing call on any sequence
        Launcher lc(seq, stream);
        SeqArgs A = seq->args();
        SeqSampling S = seq->samp;
        SeqSampleIO io = {ux, uy, it_p.x, it_p.y, it_p.z, active, ds_d.x, ds_d.y, ds_d.z, ds_pdf, ds_dist,
                          ds_p.x, ds_p.y, ds_p.z, weight, wstride};
        if (!spec) {
            void* args[] = {&lc.K, &A, &S, &io, &n};
            lc.run(K_SEQUENCE_SAMPLE_RGB, n, args);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&lc.K, &A, &S, &L, &io, &n};
            lc.run(K_SEQUENCE_SAMPLE_SPEC, n, args);
        }
    });
}

int sunsky_sequence_pdf_direction(const sunsky_sequence* seq, sunsky_vec3_in d, const uint8_t* active, size_t n,
                                  float* pdf, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_pdf_direction");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (n == 0) return SUNSKY_OK;
    if (!d.x || !d.y || !d.z || !pdf) return fail(SUNSKY_ERROR_INVALID_VALUE, "null direction / output pointer");
    return guarded([&] {
        seq->require_sampling();   // first: the message names the missing call on any sequence
        Launcher lc(seq, stream);
        SeqSampling S = seq->samp;
        int count = seq->count;
        void* args[] = {&lc.K, &S, &count, (void*)&d.x, (void*)&d.y, (void*)&d.z, &active, &n, &pdf};
        lc.run(K_SEQUENCE_PDF, n, args);
    });
}

int sunsky_sequence_prepare_irradiance(sunsky_sequence* seq, int n_z, int n_phi, const float* lam_host, int m) {
    SUNSKY_PHASE("InitScene", "sequence_prepare_irradiance");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (n_z < 1 || n_z > kSeqSampleMaxZ || n_phi < 4 || n_phi > kSeqSampleMaxPhi ||
        (int64_t)n_z * n_phi > kSeqSampleMaxCells)
        return fail(SUNSKY_ERROR_INVALID_VALUE,
                    "irradiance table size out of range: 1 <= n_z <= 1024, 4 <= n_phi <= 4096, n_z * n_phi <= 2^20");
    const bool spec = seq->variant == kSpectral;
    if (spec && (!lam_host || m < 1 || m > kSeqIrrMaxPlanes))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "1..32 wavelengths required for the irradiance tables of a spectral sequence");
    if (!spec && (lam_host || m)) return fail(SUNSKY_ERROR_INVALID_VALUE, "an RGB sequence takes no wavelengths");
    const int planes = spec ? m : 3;
    const size_t cells = (size_t)n_z * (size_t)n_phi;
    if (cells * (size_t)planes > kSeqIrrMaxValues)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "irradiance table size out of range: n_z * n_phi * n_planes <= 2^22");
    return guarded([&] {
        const int count = seq->count;
        SeqIrrTableArgs T;
        std::memset(&T, 0, sizeof(T));
        if (spec) T.L = make_lambda_set(lam_host, m);
        T.nz = n_z;
        T.nphi = n_phi;
        T.planes = planes;
        T.sin2_half_ap = 1.f / seq->kargs.inv_sin2_half_ap;
        const float omega = (float)(2.0 * 3.14159265358979323846 / (double)cells);
        std::vector<float> sky(cells * planes), flux((size_t)planes * count), image;
        std::vector<int> cols = seq_irradiance_sun_columns(seq, n_phi);
        auto accept = [&] {
            seq->irr_sun_cols = std::move(cols);
            seq->irr_sky = std::move(sky);
            seq->irr_flux = std::move(flux);
            seq->irr_omega = omega;
            seq->irr_nz = n_z;
            seq->irr_nphi = n_phi;
            seq->irr_planes = planes;
            seq->irr_L = T.L;
            if (seq->irr_grad_wanted) seq_stage_irradiance_grad(seq);   // sticky: restaged for the new tables
            // ... and so is the series (tables above its cap leave it unprepared)
            if (seq->irr_series_wanted) seq_stage_irradiance_series(seq, /*quiet=*/true);
        };
        seq->irr_grad_ready = false;
        seq->irr_series_ready = false;
        if (seq->device < 0) {
            seq_irradiance_host(seq, n_z, n_phi, T.L, planes, T.sin2_half_ap, sky, flux);
            accept();
            return;
        }
        DeviceScope g(seq->device);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // nothing may still read the old image
        seq->irr_nz = seq->irr_nphi = seq->irr_planes = 0;
        seq->d_irr.reset();
        // the image's allocation first holds the two tables the kernels write: a record has 3 floats
        // more than planes, so it is never smaller
        const size_t rec = (size_t)seq_irr_record(planes);
        const size_t image_cap = (cells + (size_t)count) * rec;
        static_assert(sizeof(int) == sizeof(float), "the suns' columns lie behind the image");
        seq->d_irr.alloc(image_cap + (size_t)count);
        float* const irr = seq->d_irr.get();
        T.sky = irr;
        T.flux = irr + sky.size();
        const SunskyKArgs* K = seq->d_state.get();
        SeqArgs A = seq->args();
        void* args[] = {&K, &A, &T};
        launch(seq->mod, K_SEQUENCE_IRRADIANCE_TABLE, grid_for(seq->mod, K_SEQUENCE_IRRADIANCE_TABLE, cells, /*tunable=*/false),
               kBlock, nullptr, args);
        launch(seq->mod, K_SEQUENCE_IRRADIANCE_FLUX, (unsigned)std::min(count, 65535), kWaveBlock, nullptr, args);
        hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
        hip_check(hipMemcpy(sky.data(), T.sky, sizeof(float) * sky.size(), hipMemcpyDeviceToHost), "hipMemcpy");
        hip_check(hipMemcpy(flux.data(), T.flux, sizeof(float) * flux.size(), hipMemcpyDeviceToHost), "hipMemcpy");
        std::vector<int> kept;
        const int nsuns = seq_irradiance_image(seq, n_z, n_phi, planes, omega, sky, flux, image, kept);
        hip_check(hipMemcpy(irr, image.data(), sizeof(float) * image.size(), hipMemcpyHostToDevice), "hipMemcpy");
        seq->irr = SeqIrradiance{irr, irr + cells * rec, n_z, n_phi, nsuns, planes};
        for (int& k : kept) k = cols[(size_t)k];   // the image's suns' columns, in its order
        seq->d_irr_sun_cols = reinterpret_cast<const int*>(irr + image_cap);
        if (nsuns)
            hip_check(hipMemcpy(irr + image_cap, kept.data(), sizeof(int) * kept.size(), hipMemcpyHostToDevice),
                      "hipMemcpy");
        accept();
    });
}

int sunsky_sequence_irradiance_info(const sunsky_sequence* seq, sunsky_sequence_irradiance_desc* out) {
    if (!seq || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    return guarded([&] {
        seq->require_irradiance();
        out->n_z = seq->irr_nz;
        out->n_phi = seq->irr_nphi;
        out->n_planes = seq->irr_planes;
        out->omega = seq->irr_omega;
    });
}

int sunsky_sequence_get_irradiance_table(const sunsky_sequence* seq, int id, float* out, size_t cap, size_t* count) {
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        seq->require_irradiance();
        const std::vector<float>* t = nullptr;
        switch (id) {
            case SUNSKY_SEQUENCE_IRRADIANCE_TABLE_SKY: t = &seq->irr_sky; break;
            case SUNSKY_SEQUENCE_IRRADIANCE_TABLE_SUN_FLUX: t = &seq->irr_flux; break;
            default: throw std::invalid_argument("unknown sequence irradiance table id");
        }
        if (count) *count = t->size();
        if (out) std::memcpy(out, t->data(), sizeof(float) * std::min(cap, t->size()));
    });
}

int sunsky_sequence_irradiance(const sunsky_sequence* seq, sunsky_vec3_in nrm, const uint8_t* active, size_t n,
                               float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_irradiance");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (n == 0) return SUNSKY_OK;
    if (!nrm.x || !nrm.y || !nrm.z || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal / output pointer");
    if (n > 0xffffffffull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 receivers");
    return guarded([&] {
        seq->require_irradiance();   // first: the message names the missing call on any sequence
        Launcher lc(seq, stream);
        if (seq->irr_planes > 1 && ostride < n) throw std::invalid_argument("out_stride < n");
        SeqIrradiance S = seq->irr;
        void* args[] = {&lc.K, &S, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &out, &ostride};
        lc.run(seq->variant == kSpectral ? K_SEQUENCE_IRRADIANCE_SPEC : K_SEQUENCE_IRRADIANCE_RGB, n, args);
    });
}

int sunsky_sequence_get_irradiance_sun_columns(const sunsky_sequence* seq, int* out, size_t cap, size_t* count) {
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        seq->require_irradiance();
        const std::vector<int>& c = seq->irr_sun_cols;
        if (count) *count = c.size();
        if (out) std::memcpy(out, c.data(), sizeof(int) * std::min(cap, c.size()));
    });
}

int sunsky_sequence_irradiance_horizon(const sunsky_sequence* seq, sunsky_vec3_in nrm, const float* horizon, int n_sectors,
                                       size_t n_profiles, size_t hstride, const uint8_t* active, size_t n, float* out,
                                       size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_irradiance_horizon");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (n == 0) return SUNSKY_OK;
    if (!nrm.x || !nrm.y || !nrm.z || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal / output pointer");
    if (!horizon) return fail(SUNSKY_ERROR_INVALID_VALUE, "null horizon pointer");
    if (n > 0xffffffffull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 receivers");
    return guarded([&] {
        seq->require_irradiance();   // first: the message names the missing call on any sequence
        if (n_sectors < 1 || seq->irr_nphi % n_sectors != 0)
            throw std::invalid_argument("n_sectors must be >= 1 and divide the irradiance tables' n_phi");
        if (n_profiles != 1 && n_profiles != n) throw std::invalid_argument("n_profiles must be 1 or n");
        if (n_profiles == n && n_sectors > 1 && hstride < n) throw std::invalid_argument("horizon_stride < n");
        if (seq->irr_planes > 1 && ostride < n) throw std::invalid_argument("out_stride < n");
        Launcher lc(seq, stream);
        SeqIrradiance S = seq->irr;
        SeqIrrHorizon Z = {horizon, seq->d_irr_sun_cols, hstride, n_sectors, seq->irr_nphi / n_sectors,
                           n_profiles == 1 ? 0 : 1, 0};
        void* args[] = {&lc.K, &S, &Z, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &out, &ostride};
        lc.run(seq->variant == kSpectral ? K_SEQUENCE_IRRADIANCE_HORIZON_SPEC : K_SEQUENCE_IRRADIANCE_HORIZON_RGB, n, args);
    });
}

int sunsky_sequence_prepare_irradiance_series(sunsky_sequence* seq) {
    SUNSKY_PHASE("InitScene", "sequence_prepare_irradiance_series");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        seq->require_irradiance();
        DeviceScope g(seq->device);   // host-only (-1): no device to scope
        // nothing may still read the old images
        if (seq->device >= 0) hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        seq_stage_irradiance_series(seq);
        seq->irr_series_wanted = true;
    });
}

int sunsky_sequence_get_irradiance_frame_table(const sunsky_sequence* seq, int k, float* out, size_t cap, size_t* count) {
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        seq->require_irradiance();
        if (k < 0 || k >= seq->count) throw std::invalid_argument("frame index out of range");
        const size_t total = (size_t)seq->irr_planes * (size_t)seq->irr_nz * (size_t)seq->irr_nphi;
        if (count) *count = total;
        if (!out || !cap) return;
        std::vector<float> t(total, 0.f);
        if (seq->device < 0) {
            seq_irradiance_sky_host(seq, seq->irr_nz, seq->irr_nphi, seq->irr_L, seq->irr_planes, k, k + 1, /*unit=*/true,
                                    t.data());
        } else {
            DeviceScope g(seq->device);
            DeviceBuffer<float> d;
            d.alloc(total);
            hip_check(hipMemset(d.get(), 0, sizeof(float) * total), "hipMemset");
            seq_irr_series_table(seq, nullptr, d.get(), 1, 1, k);
            hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
            hip_check(hipMemcpy(t.data(), d.get(), sizeof(float) * total, hipMemcpyDeviceToHost), "hipMemcpy");
        }
        std::memcpy(out, t.data(), sizeof(float) * std::min(cap, total));
    });
}

int sunsky_sequence_irradiance_series(const sunsky_sequence* seq, sunsky_vec3_in nrm, const float* horizon, int n_sectors,
                                      size_t n_profiles, size_t hstride, const uint8_t* active, size_t n, int first_frame,
                                      int n_frames, float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_irradiance_series");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (n == 0 || n_frames == 0) return SUNSKY_OK;
    if (!nrm.x || !nrm.y || !nrm.z || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal / output pointer");
    if (n > 0xffffffffull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 receivers");
    return guarded([&] {
        seq->require_irradiance_series();   // first: the message names the missing call on any sequence
        if (first_frame < 0 || n_frames < 0 || (long long)first_frame + n_frames > seq->count)
            throw std::invalid_argument("frame range out of range: 0 <= first_frame, 0 <= n_frames, first_frame + n_frames <= count");
        if (horizon) {
            if (n_sectors < 1 || seq->irr_nphi % n_sectors != 0)
                throw std::invalid_argument("n_sectors must be >= 1 and divide the irradiance tables' n_phi");
            if (n_profiles != 1 && n_profiles != n) throw std::invalid_argument("n_profiles must be 1 or n");
            if (n_profiles == n && n_sectors > 1 && hstride < n) throw std::invalid_argument("horizon_stride < n");
        }
        const int planes = seq->irr_planes, G = seq_irr_series_group(planes);
        if ((long long)n_frames * planes > 1 && ostride < n) throw std::invalid_argument("out_stride < n");
        Launcher lc(seq, stream);
        SeqIrrSeries S = seq->irr_series;
        S.plane0 = (long long)first_frame * planes;
        S.n_planes = (long long)n_frames * planes;
        S.group0 = first_frame / G;
        S.n_groups = (first_frame + n_frames - 1) / G - S.group0 + 1;
        // one workgroup per work item (tile of receiver pairs, group), grid-stride over the items
        const size_t pairs = (n + 1) / 2, tiles = (pairs + kBlock - 1) / kBlock, items = tiles * (size_t)S.n_groups;
        const bool spec = seq->variant == kSpectral;
        if (!horizon) {
            void* args[] = {&lc.K, &S, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &out, &ostride};
            lc.run(spec ? K_SEQUENCE_IRRADIANCE_SERIES_SPEC : K_SEQUENCE_IRRADIANCE_SERIES_RGB, items * kBlock, args);
        } else {
            SeqIrrHorizon Z = {horizon, nullptr, hstride, n_sectors, seq->irr_nphi / n_sectors, n_profiles == 1 ? 0 : 1, 0};
            void* args[] = {&lc.K, &S, &Z, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &out, &ostride};
            lc.run(spec ? K_SEQUENCE_IRRADIANCE_SERIES_HORIZON_SPEC : K_SEQUENCE_IRRADIANCE_SERIES_HORIZON_RGB, items * kBlock,
                   args);
        }
    });
}

int sunsky_sequence_prepare_irradiance_grad(sunsky_sequence* seq) {
    SUNSKY_PHASE("InitScene", "sequence_prepare_irradiance_grad");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        seq->require_irradiance();
        DeviceScope g(seq->device);   // host-only (-1): no device to scope
        // nothing may still use the old workspace
        if (seq->device >= 0) hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        seq_stage_irradiance_grad(seq);
        seq->irr_grad_wanted = true;
    });
}

int sunsky_sequence_irradiance_vjp(const sunsky_sequence* seq, sunsky_vec3_in nrm, const uint8_t* active, size_t n,
                                   const float* d_out, size_t d_stride, sunsky_vec3_out grad_normal, float* grad_weight,
                                   void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_irradiance_vjp");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (n == 0) return SUNSKY_OK;
    if (!nrm.x || !nrm.y || !nrm.z || !d_out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal / d_out pointer");
    if (int rc = check_optional_vec3(grad_normal, "grad_normal")) return rc;
    if (n > 0xffffff00ull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 - 256 receivers");
    return guarded([&] {
        seq->require_irradiance_grad();   // first: the message names the missing call on any sequence
        Launcher lc(seq, stream);
        if (seq->irr_planes > 1 && d_stride < n) throw std::invalid_argument("d_stride < n");
        SeqIrradiance S = seq->irr;
        const bool spec = seq->variant == kSpectral;
        if (grad_normal.x) {
            void* args[] = {&lc.K, &S, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &d_out, &d_stride,
                            (void*)&grad_normal.x, (void*)&grad_normal.y, (void*)&grad_normal.z};
            lc.run(spec ? K_SEQUENCE_IRRADIANCE_VJP_NORMAL_SPEC : K_SEQUENCE_IRRADIANCE_VJP_NORMAL_RGB, n, args);
        }
        if (!grad_weight) return;
        const size_t cells = (size_t)seq->irr_nz * (size_t)seq->irr_nphi, entries = cells + (size_t)seq->count;
        const SeqIrrGradShape shape = seq_irr_grad_shape(n, seq->irr_planes, cells, seq->count, seq->irr_grad_cap);
        SeqIrrGrad G = seq->irr_grad;
        G.dout = d_out;
        G.dstride = d_stride;
        G.slices = shape.slices;
        G.slice_len = shape.slice_len;
        const size_t tiles = (entries + kSeqIrrGradTile - 1) / kSeqIrrGradTile;
        const size_t passes = spec ? (size_t)(seq->irr_planes + kSeqIrrGradSpecPlanes - 1) / kSeqIrrGradSpecPlanes : 1;
        {   // one workgroup per work item (slice, tile, pass), grid-stride over the items
            void* args[] = {&lc.K, &S, &G, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n};
            lc.run(K_SEQUENCE_IRRADIANCE_ADJOINT, (size_t)shape.slices * tiles * passes * kBlock, args);
        }
        SeqArgs A = seq->args();
        LambdaSet L = seq->irr_L;
        for (int phase = shape.slices > 1 ? 0 : 1; phase < 2; ++phase) {
            void* args[] = {&lc.K, &A, &S, &G, &L, &phase, &grad_weight};
            lc.run(K_SEQUENCE_IRRADIANCE_GRAD_FOLD, phase == 0 ? (size_t)seq->irr_planes * entries : (size_t)seq->count * kBlock,
                   args);
        }
    });
}

int sunsky_sequence_irradiance_horizon_vjp(const sunsky_sequence* seq, sunsky_vec3_in nrm, const float* horizon, int n_sectors,
                                           size_t n_profiles, size_t hstride, const uint8_t* active, size_t n,
                                           const float* d_out, size_t d_stride, sunsky_vec3_out grad_normal,
                                           float* grad_weight, float* grad_horizon, size_t ghstride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_irradiance_horizon_vjp");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (n == 0) return SUNSKY_OK;
    if (!nrm.x || !nrm.y || !nrm.z || !d_out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal / d_out pointer");
    if (int rc = check_optional_vec3(grad_normal, "grad_normal")) return rc;
    if (n > 0xffffff00ull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 - 256 receivers");
    if (!horizon) return fail(SUNSKY_ERROR_INVALID_VALUE, "null horizon pointer");
    if (n_sectors < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "n_sectors must be >= 1 and divide the irradiance tables' n_phi");
    if (n_profiles != 1 && n_profiles != n) return fail(SUNSKY_ERROR_INVALID_VALUE, "n_profiles must be 1 or n");
    if (n_profiles == n && n_sectors > 1 && hstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "horizon_stride < n");
    if (grad_horizon && n_sectors > 1 && ghstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "grad_horizon_stride < n");
    return guarded([&] {
        seq->require_irradiance_grad();   // the message names the missing call on any sequence
        if (seq->irr_nphi % n_sectors != 0)
            throw std::invalid_argument("n_sectors must be >= 1 and divide the irradiance tables' n_phi");
        Launcher lc(seq, stream);
        if (seq->irr_planes > 1 && d_stride < n) throw std::invalid_argument("d_stride < n");
        SeqIrradiance S = seq->irr;
        SeqIrrHorizon Z = {horizon, seq->d_irr_sun_cols, hstride, n_sectors, seq->irr_nphi / n_sectors,
                           n_profiles == 1 ? 0 : 1, 0};
        const bool spec = seq->variant == kSpectral;
        if (grad_normal.x) {
            void* args[] = {&lc.K, &S, &Z, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &d_out, &d_stride,
                            (void*)&grad_normal.x, (void*)&grad_normal.y, (void*)&grad_normal.z};
            lc.run(spec ? K_SEQUENCE_IRRADIANCE_HORIZON_VJP_NORMAL_SPEC : K_SEQUENCE_IRRADIANCE_HORIZON_VJP_NORMAL_RGB, n, args);
        }
        if (grad_horizon) {
            void* args[] = {&lc.K, &S, &Z, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &d_out, &d_stride,
                            &grad_horizon, &ghstride};
            lc.run(spec ? K_SEQUENCE_IRRADIANCE_HORIZON_VJP_PROFILE_SPEC : K_SEQUENCE_IRRADIANCE_HORIZON_VJP_PROFILE_RGB, n, args);
        }
        if (!grad_weight) return;
        const size_t cells = (size_t)seq->irr_nz * (size_t)seq->irr_nphi, entries = cells + (size_t)seq->count;
        const SeqIrrGradShape shape = seq_irr_grad_shape(n, seq->irr_planes, cells, seq->count, seq->irr_grad_cap);
        SeqIrrGrad G = seq->irr_grad;
        G.dout = d_out;
        G.dstride = d_stride;
        G.slices = shape.slices;
        G.slice_len = shape.slice_len;
        Z.sun_cols = seq->d_irr_grad_cols;   // all K frames' columns
        const size_t units = seq_irr_hz_grad_units(seq->irr_nz, Z.sector_len, n_sectors, seq->count);
        const size_t passes = spec ? (size_t)(seq->irr_planes + kSeqIrrGradSpecPlanes - 1) / kSeqIrrGradSpecPlanes : 1;
        {   // one workgroup per work item (slice, unit, pass), grid-stride over the items
            void* args[] = {&lc.K, &S, &G, &Z, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n};
            lc.run(K_SEQUENCE_IRRADIANCE_HORIZON_ADJOINT, (size_t)shape.slices * units * passes * kBlock, args);
        }
        SeqArgs A = seq->args();
        LambdaSet L = seq->irr_L;
        for (int phase = shape.slices > 1 ? 0 : 1; phase < 2; ++phase) {
            void* args[] = {&lc.K, &A, &S, &G, &L, &phase, &grad_weight};
            lc.run(K_SEQUENCE_IRRADIANCE_GRAD_FOLD, phase == 0 ? (size_t)seq->irr_planes * entries : (size_t)seq->count * kBlock,
                   args);
        }
    });
}

}  // extern "C"
