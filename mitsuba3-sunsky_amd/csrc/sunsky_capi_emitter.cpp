// sunsky_capi_emitter.cpp -- the emitter half of the C ABI (include/sunsky_amd.h): props,
// the emitter handle (host staging through SunskyModel, device tables), and its eval,
// sampling, AD, bake and direct-lighting entry points.
#include "sunsky_launch.h"
#include "sunsky_props.h"

using namespace sunsky;
using namespace sunsky::capi;

// ---------------------------------------------------------------- handles
struct sunsky_props {
    Properties props;
};

struct sunsky_emitter {
    DrainOnDestroy drain;   // first: destroyed after every owner below (sunsky_launch.h)
    std::unique_ptr<SunskyModel> model;
    // Host mirror of the state: geometry, dispatch fields (variant, semantics, nch) and,
    // once read back (sync_host), the device-staged radiance fields.
    SunskyKArgs kargs;
    DeviceModule* mod = nullptr;
    int device = 0;
    int precision = SUNSKY_PRECISION_FAST;
    // ---- device state (one per emitter per GPU).  Every kernel reads the emitter
    // through `d_state` (SunskyKArgs in device memory, s_load'ed by the kernels);
    // parameters_changed rewrites it in place, ordered on the caller's stream.
    DeviceBuffer<SunskyKArgs> d_state;
    DeviceBuffer<float> d_sun_table, d_sun_ld;
    DeviceBuffer<float> d_datasets;       // sky params | sky radiance | sun table | quadrature x | w
    const float *d_sky_params_ds = nullptr, *d_sky_rad_ds = nullptr, *d_sun_rad_ds = nullptr;
    const float *d_qx = nullptr, *d_qw = nullptr;
    DeviceBuffer<float> d_quad_part;      // quadrature row sums [2][200][nch]
    DeviceBuffer<int> d_status;           // device staging status (0 ok)
    static constexpr int kRing = 4;       // pinned host images of the state for the async copy
    PinnedBuffer<SunskyKArgs> h_ring;
    DeviceEvent ring_ev[kRing];
    bool ring_used[kRing] = {};
    int ring_i = 0;
    bool restoring = false;                    // restaging the accepted state after a rejection
    int inject_faults = 0;                     // testing: stagings left that report a rejection
    DeviceEvent stage_done;                    // recorded after the last device staging
    mutable DeviceBuffer<float> d_jvp;   // eval_jvp tangent tables (layout: sunsky_kernels.hip)
    mutable DeviceBuffer<float> d_vjp;   // eval_vjp basis-tangent tables
    // AD tangent tables depend only on the emitter state: restaged when `rev` (bumped by
    // every staging) or, for the JVP, the requested tangent changes.  `ad` holds eval_vjp's
    // per-workgroup gradient partials and orders every AD call after the previous one, so a
    // later call on another stream cannot overwrite d_jvp / d_vjp / the partials under an
    // in-flight kernel.  The bakes order their angle tables the same way (`bake`).
    uint64_t rev = 0;
    mutable uint64_t vjp_rev = ~0ull, jvp_rev = ~0ull;
    mutable std::vector<float> jvp_key;
    mutable OrderedScratch<float> ad, bake;

    static constexpr int kJvpFloats = kJvpSunOffset + kSunRgbTableSize;   // AD tangent buffers
    static constexpr int kVjpFloats = kVjpSunOffset + kSunRgbTableSize;

    // Allocations of a GPU emitter (once, at creation): state, tables, the raw datasets
    // the staging kernels read, quadrature nodes, scratch, pinned ring, events.
    void init_device() {
        const bool spec = model->variant() == kSpectral;
        d_state.alloc(1);
        d_sun_table.alloc(kSunRgbTableSize);
        d_sun_ld.alloc(kNbWavelengths * kNbSunLdParams);
        const std::vector<float>& sp = model->sky_params_ds();
        const std::vector<float>& sr = model->sky_rad_ds();
        const std::vector<float>& su = model->sun_rad_ds();
        std::vector<float> qx, qw;
        SunskyModel::quadrature_nodes(&qx, &qw);
        std::vector<float> all;
        all.reserve(sp.size() + sr.size() + su.size() + qx.size() + qw.size());
        all.insert(all.end(), sp.begin(), sp.end());
        all.insert(all.end(), sr.begin(), sr.end());
        all.insert(all.end(), su.begin(), su.end());
        all.insert(all.end(), qx.begin(), qx.end());
        all.insert(all.end(), qw.begin(), qw.end());
        d_datasets.alloc(all.size());
        hip_check(hipMemcpy(d_datasets.get(), all.data(), sizeof(float) * all.size(), hipMemcpyHostToDevice), "hipMemcpy");
        d_sky_params_ds = d_datasets.get();
        d_sky_rad_ds = d_sky_params_ds + sp.size();
        d_sun_rad_ds = d_sky_rad_ds + sr.size();
        d_qx = d_sun_rad_ds + su.size();
        d_qw = d_qx + qx.size();
        const std::vector<float>& ld = model->sun_ld();
        if (spec)
            hip_check(hipMemcpy(d_sun_ld.get(), ld.data(), sizeof(float) * std::min<size_t>(ld.size(), d_sun_ld.size()),
                                hipMemcpyHostToDevice), "hipMemcpy");
        d_quad_part.alloc(2 * qx.size() * model->nch());
        d_status.alloc(1);
        hip_check(hipMemset(d_status.get(), 0, sizeof(int)), "hipMemset");
        h_ring.alloc(kRing);
        for (DeviceEvent& ev : ring_ev) ev.create();
        stage_done.create();
    }

    // parameters_changed on the device, ordered on `s`: the host-staged part of the
    // state (geometry, TGMM, discrete distribution) by an async copy from a pinned image,
    // then the staging kernels write the sky channels, the sun table and (JIT) the
    // sampling weight and wavelength distribution.  Nothing here waits for the device,
    // except for a pinned image still in flight kRing updates later.
    void stage_async(hipStream_t s) {
        kargs = model->kargs();
        kargs.sun_table = d_sun_table.get();
        kargs.sun_ld = d_sun_ld.get();
        const int slot = ring_i;
        ring_i = (ring_i + 1) % kRing;
        if (ring_used[slot]) hip_check(hipEventSynchronize(ring_ev[slot].get()), "hipEventSynchronize");
        h_ring.get()[slot] = kargs;
        hip_check(hipMemcpyAsync(d_state.get(), &h_ring.get()[slot], sizeof(SunskyKArgs), hipMemcpyHostToDevice, s),
                  "hipMemcpyAsync");
        hip_check(hipEventRecord(ring_ev[slot].get(), s), "hipEventRecord");
        ring_used[slot] = true;
        const bool spec = model->variant() == kSpectral;
        StageArgs A;
        std::memset(&A, 0, sizeof(A));
        A.state = d_state.get();
        A.sun_table = d_sun_table.get();
        A.sky_params_ds = d_sky_params_ds;
        A.sky_rad_ds = d_sky_rad_ds;
        A.sun_rad_ds = d_sun_rad_ds;
        A.rs = model->radiance_stage();
        const std::vector<float>& alb = model->albedo();
        for (int c = 0; c < model->nch(); ++c) A.albedo[c] = alb[c];
        A.nch = model->nch();
        A.variant = model->variant();
        A.sun_block = spec ? kSunSpecTableSize : kSunRgbTableSize;
        A.sky_scale = model->sky_scale();
        void* sargs[] = {&A};
        launch(mod, K_STAGE_RADIANCE, 1, kBlock, s, sargs);
        if (model->semantics() == kJit) {
            QuadArgs Q;
            std::memset(&Q, 0, sizeof(Q));
            Q.state = d_state.get();
            Q.qx = d_qx;
            Q.qw = d_qw;
            Q.rows = d_quad_part.get();
            Q.nq = 200;
            Q.nch = model->nch();
            std::memcpy(Q.cie_y, model->cie_y(), sizeof(Q.cie_y));
            Q.sky_scale = model->sky_scale();
            Q.sun_scale = model->sun_scale();
            Q.status = d_status.get();
            void* qargs[] = {&Q};
            static_assert(200 <= kQuadBlock, "one quadrature row per workgroup");
            launch(mod, K_STAGE_QUAD_POINTS, (unsigned)Q.nq, kQuadBlock, s, qargs);
            launch(mod, K_STAGE_QUAD_FINISH, 1, kBlock, s, qargs);
        }
        if (inject_faults > 0 && model->semantics() == kJit && !restoring) {   // sunsky_emitter_inject_staging_fault
            --inject_faults;
            hip_check(hipMemsetAsync(d_status.get(), 1, 1, s), "hipMemsetAsync");
        }
        hip_check(hipEventRecord(stage_done.get(), s), "hipEventRecord");
        ++rev;
    }

    // Bring the device-staged fields back into the host model (get_info / get_table /
    // to_string): waits for the last staging only.
    void sync_host() const {
        if (!model->radiance_stale() || !d_state.get()) return;
        DeviceScope g(device);
        hip_check(hipEventSynchronize(stage_done.get()), "hipEventSynchronize");
        SunskyKArgs dk;
        hip_check(hipMemcpy(&dk, d_state.get(), sizeof(dk), hipMemcpyDeviceToHost), "hipMemcpy");
        std::vector<float> st(kSunRgbTableSize);
        hip_check(hipMemcpy(st.data(), d_sun_table.get(), sizeof(float) * st.size(), hipMemcpyDeviceToHost), "hipMemcpy");
        int status = 0;
        hip_check(hipMemcpy(&status, d_status.get(), sizeof(int), hipMemcpyDeviceToHost), "hipMemcpy");
        auto* self = const_cast<sunsky_emitter*>(this);
        if (status) {
            // A device staging since the last read-back rejected its update (a negative
            // wavelength-distribution node, the check of ContinuousDistribution's
            // constructor); the status is sticky, so which one is unknown.  As the reference
            // throws from parameters_changed and keeps its old state: restore the parameters
            // of the last staging known to be accepted, restage them, report the error once.
            hip_check(hipMemset(d_status.get(), 0, sizeof(int)), "hipMemset");
            if (restoring || !model->has_accepted())   // the accepted state itself is rejected (e.g. at creation)
                throw std::runtime_error("ContinuousDistribution: entries must be non-negative!");
            model->revert_to_accepted();
            self->restoring = true;
            try {
                // batch kernels queued on any stream may still read d_state: let them drain
                // before it is rewritten (a rare error path; no stream of the caller is known)
                hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
                self->stage_async(nullptr);
                hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
                sync_host();
            } catch (...) {
                self->restoring = false;
                throw;
            }
            self->restoring = false;
            throw std::runtime_error("ContinuousDistribution: entries must be non-negative! (update rejected by the "
                                     "device staging; the parameters of the last accepted update were restored)");
        }
        model->mark_accepted();
        model->adopt_device_stage(dk, st.data());
        const SunskyKArgs& hk = model->kargs();
        std::memcpy(self->kargs.sky, hk.sky, sizeof(hk.sky));
        std::memcpy(self->kargs.fsky, hk.fsky, sizeof(hk.fsky));
        self->kargs.w_sky = hk.w_sky;
        self->kargs.sun_sky_fit_on = hk.sun_sky_fit_on;
        self->kargs.spec_size = hk.spec_size;
        std::memcpy(self->kargs.spec_pdf, hk.spec_pdf, sizeof(hk.spec_pdf));
        std::memcpy(self->kargs.spec_cdf, hk.spec_cdf, sizeof(hk.spec_cdf));
        self->kargs.spec_integral = hk.spec_integral;
        self->kargs.spec_norm = hk.spec_norm;
        self->kargs.spec_interval = hk.spec_interval;
        self->kargs.spec_inv_interval = hk.spec_inv_interval;
    }

    // the identity-to_world code object for emitters whose to_world is the identity
    // (SUNSKY_AMD_GENERAL_XFORM=1: the general one always; the bitwise test of the two)
    // A launch being captured into a hipGraph takes the general code object: the graph may be
    // replayed after an update that gives the emitter a non-identity to_world (captured
    // launches read the current state), which the identity kernels would not apply.
    int xform_form(hipStream_t s) const {
        if (!kargs.identity_xform || general_xform()) return 0;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        hip_check(hipStreamIsCapturing(s, &cs), "hipStreamIsCapturing");
        return cs == hipStreamCaptureStatusNone ? 1 : 0;
    }
    // Batch calls need the emitter's device state: a host-only emitter
    // (sunsky_emitter_create_host) has none and rejects them.
    void require_device() const {
        if (!mod) throw std::invalid_argument("host-only emitter (sunsky_emitter_create_host) cannot launch kernels");
    }

    // the owners free what they hold once this body has run: device current, launches drained
    ~sunsky_emitter() { drain.enter(device); }

    // Device tangent staging into an AD table buffer (sunsky_stage_tangent, sunsky_staging.h):
    // the arguments for `nbasis` bases over this emitter's datasets, then the launch.
    TangentArgs tangent_args(float* out, int nbasis, int sun_local_off, int sun_local_first, int sun_off,
                             int total) const {
        TangentArgs A;
        std::memset(&A, 0, sizeof(A));
        A.sky_params_ds = d_sky_params_ds;
        A.sky_rad_ds = d_sky_rad_ds;
        A.sun_rad_ds = d_sun_rad_ds;
        A.out = out;
        A.nbasis = A.nsky = nbasis;
        A.sun_local_off = sun_local_off;
        A.sun_local_first = sun_local_first;
        A.sun_off = sun_off;
        A.sun_block = model->variant() == kSpectral ? kSunSpecTableSize : kSunRgbTableSize;
        A.total = total;
        return A;
    }
    void stage_tangent(TangentArgs& A, hipStream_t st) const {
        void* args[] = {&A};
        launch(mod, K_STAGE_TANGENT, (unsigned)((A.total + kBlock - 1) / kBlock), kBlock, st, args);
    }
};

EmitterSnapshot sunsky::capi::emitter_snapshot(const sunsky_emitter* e) {
    return {*e->model, e->kargs, e->mod, e->device, e->precision};
}

extern "C" {

int sunsky_props_create(sunsky_props** out) {
    if (!out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null output pointer");
    return guarded([&] { *out = new sunsky_props(); });
}
void sunsky_props_destroy(sunsky_props* p) { delete p; }

#define PROPS_GUARD(p, name)                                                                   \
    if (!(p) || !(name)) return fail(SUNSKY_ERROR_INVALID_VALUE, "null props / property name")

int sunsky_props_set_float(sunsky_props* p, const char* name, double v) {
    PROPS_GUARD(p, name);
    return guarded([&] { p->props.set_float(name, v); });
}
int sunsky_props_set_int(sunsky_props* p, const char* name, int64_t v) {
    PROPS_GUARD(p, name);
    return guarded([&] { p->props.set_int(name, v); });
}
int sunsky_props_set_vector3(sunsky_props* p, const char* name, float x, float y, float z) {
    PROPS_GUARD(p, name);
    return guarded([&] { p->props.set_vector3(name, x, y, z); });
}
int sunsky_props_set_transform(sunsky_props* p, const char* name, const float m[16]) {
    PROPS_GUARD(p, name);
    if (!m) return fail(SUNSKY_ERROR_INVALID_VALUE, "null matrix");
    return guarded([&] { p->props.set_transform(name, m); });
}
int sunsky_props_set_spectrum(sunsky_props* p, const char* name, const float* v, int n) {
    PROPS_GUARD(p, name);
    if (!v || n <= 0) return fail(SUNSKY_ERROR_INVALID_VALUE, "empty spectrum");
    return guarded([&] { p->props.set_spectrum(name, v, n); });
}
int sunsky_props_set_irregular_spectrum(sunsky_props* p, const char* name, const float* wl, const float* v, int n) {
    PROPS_GUARD(p, name);
    if (!wl || !v || n <= 0) return fail(SUNSKY_ERROR_INVALID_VALUE, "empty spectrum");
    return guarded([&] { p->props.set_irregular(name, wl, v, n); });
}

int sunsky_emitter_create(const sunsky_props* props, int variant, int semantics, const char* dataset_path,
                          sunsky_emitter** out) {
    SUNSKY_PHASE("InitScene", "emitter_create");
    if (!props || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null props / output pointer");
    *out = nullptr;
    return guarded([&] {
        std::unique_ptr<sunsky_emitter> e(new sunsky_emitter());
        std::string ds = dataset_path && *dataset_path ? std::string(dataset_path) : default_pack_path();
        // radiance tables + quadrature are staged on the device (stage_async)
        e->model.reset(new SunskyModel(props->props, variant, semantics, ds, /*radiance_on_host=*/false));
        hip_check(hipGetDevice(&e->device), "hipGetDevice");
        e->mod = module_for_device(e->device);
        if (const char* env = std::getenv("SUNSKY_AMD_PRECISION"))
            e->precision = std::strcmp(env, "reference") == 0 ? SUNSKY_PRECISION_REFERENCE : SUNSKY_PRECISION_FAST;
        e->init_device();
        e->stage_async(nullptr);
        hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
        e->sync_host();
        for (const std::string& w : e->model->warnings) std::fprintf(stderr, "WARN sunsky: %s\n", w.c_str());
        *out = e.release();
    });
}

int sunsky_emitter_create_host(const sunsky_props* props, int variant, int semantics, const char* dataset_path,
                               sunsky_emitter** out) {
    if (!props || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null props / output pointer");
    *out = nullptr;
    return guarded([&] {
        std::unique_ptr<sunsky_emitter> e(new sunsky_emitter());
        std::string ds = dataset_path && *dataset_path ? std::string(dataset_path) : default_pack_path();
        e->model.reset(new SunskyModel(props->props, variant, semantics, ds));
        e->device = -1;
        e->kargs = e->model->kargs();
        *out = e.release();
    });
}

void sunsky_emitter_destroy(sunsky_emitter* e) { delete e; }

int sunsky_emitter_set_param(sunsky_emitter* e, const char* name, const float* v, int count) {
    if (!e || !name || !v) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    return guarded([&] { e->model->set_param(name, v, count); });
}

int sunsky_emitter_parameters_changed_async(sunsky_emitter* e, void* stream) {
    SUNSKY_PHASE("InitScene", "emitter_parameters_changed_async");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    return guarded([&] {
        const bool gpu = e->device >= 0;
        if (gpu) {
            // The update is a host + stream operation (pinned-image copy, events), not a
            // graph node: refuse it during capture before anything is committed or queued.
            DeviceScope g(e->device);
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            hip_check(hipStreamIsCapturing((hipStream_t)stream, &cs), "hipStreamIsCapturing");
            if (cs != hipStreamCaptureStatusNone) {
                e->model->discard_pending();
                throw std::invalid_argument("parameters_changed cannot be captured into a hipGraph: update the "
                                            "emitter outside the capture (a captured graph reads the current state)");
            }
        }
        e->model->parameters_changed(/*radiance_on_host=*/!gpu);   // keeps the scene bounding sphere
        if (gpu) {
            DeviceScope g(e->device);
            e->stage_async((hipStream_t)stream);
        } else {
            e->kargs = e->model->kargs();
        }
    });
}

int sunsky_emitter_inject_staging_fault(sunsky_emitter* e, int count) {
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (count < 0) return fail(SUNSKY_ERROR_INVALID_VALUE, "count must be >= 0");
    e->inject_faults = count;
    return SUNSKY_OK;
}

int sunsky_emitter_sun_segments(const sunsky_emitter* e, const float* cos_theta, size_t n, int* pos, void* stream) {
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (n == 0) return SUNSKY_OK;
    if (!cos_theta || !pos) return fail(SUNSKY_ERROR_INVALID_VALUE, "null input / output pointer");
    return guarded([&] {
        Launcher lc(e, stream);
        void* args[] = {&lc.K, &cos_theta, &n, &pos};
        lc.run(K_DEBUG_SUN_SEGMENTS, n, args);
    });
}

int sunsky_emitter_parameters_changed(sunsky_emitter* e) {
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    int rc = sunsky_emitter_parameters_changed_async(e, nullptr);
    if (rc != SUNSKY_OK || e->device < 0) return rc;
    return guarded([&] {
        DeviceScope g(e->device);
        hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
        e->sync_host();
    });
}

int sunsky_emitter_get_param(const sunsky_emitter* e, const char* name, float* out, int cap, int* count) {
    if (!e || !name || !count) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    return guarded([&] { *count = e->model->get_param(name, out, out ? cap : 0); });
}

int sunsky_emitter_set_scene(sunsky_emitter* e, int bbox_valid, const float center[3], float radius) {
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    float zero[3] = {0, 0, 0};
    return guarded([&] {
        e->model->set_scene(bbox_valid != 0, center ? center : zero, radius);
        const SunskyKArgs& k = e->model->kargs();
        std::memcpy(e->kargs.bs_center, k.bs_center, sizeof(k.bs_center));
        e->kargs.bs_radius = k.bs_radius;
        if (e->device >= 0) {   // the 4 bounding-sphere floats of the device state, in place
            DeviceScope g(e->device);
            static_assert(offsetof(SunskyKArgs, bs_radius) == offsetof(SunskyKArgs, bs_center) + 3 * sizeof(float),
                          "bounding sphere layout");
            float bs[4] = {k.bs_center[0], k.bs_center[1], k.bs_center[2], k.bs_radius};
            // a staging still queued on another stream copies the whole state block (with
            // the old sphere): let it land first, then write the sphere in place
            hip_check(hipEventSynchronize(e->stage_done.get()), "hipEventSynchronize");
            hip_check(hipMemcpy((char*)e->d_state.get() + offsetof(SunskyKArgs, bs_center), bs, sizeof(bs),
                                hipMemcpyHostToDevice), "hipMemcpy");
        }
    });
}

int sunsky_emitter_set_precision(sunsky_emitter* e, int precision) {
    if (!e || (precision != SUNSKY_PRECISION_FAST && precision != SUNSKY_PRECISION_REFERENCE))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "invalid precision mode");
    e->precision = precision;
    return SUNSKY_OK;
}

int sunsky_emitter_get_info(const sunsky_emitter* e, sunsky_info* out) {
    if (!e || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    int rc = guarded([&] { e->sync_host(); });
    if (rc != SUNSKY_OK) return rc;
    const SunskyKArgs& k = e->kargs;
    std::memset(out, 0, sizeof(*out));
    out->variant = e->model->variant();
    out->semantics = k.semantics;
    out->nb_channels = e->model->nch();
    out->active_record = e->model->active_record();
    out->turbidity = e->model->turbidity();
    out->sky_scale = k.sky_scale;
    out->sun_scale = k.sun_scale;
    out->sun_half_aperture = k.half_aperture;
    out->cos_cutoff = k.cos_cutoff;
    out->area_ratio = k.area_ratio;
    std::memcpy(out->sun_dir_world, e->model->sun_dir_world(), 3 * sizeof(float));
    std::memcpy(out->sun_dir_local, k.sun_n, 3 * sizeof(float));
    out->sun_angles[0] = k.sun_phi;
    out->sun_angles[1] = k.sun_theta;
    out->sky_sampling_w = k.w_sky;
    std::memcpy(out->bsphere_center, k.bs_center, 3 * sizeof(float));
    out->bsphere_radius = k.bs_radius;
    out->flags = SUNSKY_FLAG_INFINITE | SUNSKY_FLAG_SPATIALLY_VARYING;
    out->device = e->device;
    out->precision = e->precision;
    return SUNSKY_OK;
}

int sunsky_emitter_get_table(const sunsky_emitter* e, int id, float* out, size_t cap, size_t* count) {
    if (!e || !count) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    int rc = guarded([&] { e->sync_host(); });
    if (rc != SUNSKY_OK) return rc;
    std::vector<float> v;
    const SunskyKArgs& k = e->kargs;
    switch (id) {
        case SUNSKY_TABLE_SKY_PARAMS: v = e->model->sky_params(); break;
        case SUNSKY_TABLE_SKY_RADIANCE: v = e->model->sky_radiance(); break;
        case SUNSKY_TABLE_SUN_RADIANCE: v = e->model->sun_table(); break;
        case SUNSKY_TABLE_SUN_LD: v = e->model->sun_ld(); break;
        case SUNSKY_TABLE_GAUSSIANS: v.assign(e->model->gaussians_raw(), e->model->gaussians_raw() + kNbMixture * kNbGaussianParams); break;
        case SUNSKY_TABLE_GAUSSIAN_CDF: v.assign(k.gauss_cdf, k.gauss_cdf + kNbMixture); break;
        case SUNSKY_TABLE_SPECTRAL_PDF: v.assign(k.spec_pdf, k.spec_pdf + k.spec_size); break;
        case SUNSKY_TABLE_SPECTRAL_CDF: v.assign(k.spec_cdf, k.spec_cdf + std::max(0, k.spec_size - 1)); break;
        case SUNSKY_TABLE_ALBEDO: v = e->model->albedo(); break;
        case SUNSKY_TABLE_SUN_SKY_FIT:
            v.assign(k.sun_sky_fit, k.sun_sky_fit + 6);
            v.insert(v.end(), {k.sun_sky_fit_dev, k.sun_sky_fit_fmin, (float)k.sun_sky_fit_ok, (float)k.sun_sky_fit_on});
            break;
        case SUNSKY_TABLE_SUN_SEGMENTS:
            v.assign(k.sun_seg_z, k.sun_seg_z + kNbSunSegments);
            v.insert(v.end(), {(float)k.sun_row_lo, (float)k.sun_row_hi});
            break;
        default: return fail(SUNSKY_ERROR_INVALID_VALUE, "unknown table id");
    }
    *count = v.size();
    if (out && !v.empty()) std::memcpy(out, v.data(), sizeof(float) * std::min(cap, v.size()));
    return SUNSKY_OK;
}

int sunsky_emitter_to_string(const sunsky_emitter* e, char* buf, size_t cap) {
    if (!e || !buf || !cap) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    int rc = guarded([&] { e->sync_host(); });
    if (rc != SUNSKY_OK) return rc;
    std::string s = e->model->to_string();
    std::snprintf(buf, cap, "%s", s.c_str());
    return SUNSKY_OK;
}

int sunsky_emitter_bbox(const sunsky_emitter* e, float mn[3], float mx[3]) {
    if (!e || !mn || !mx) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    for (int i = 0; i < 3; ++i) { mn[i] = INFINITY; mx[i] = -INFINITY; }
    return SUNSKY_OK;
}

// ---------------------------------------------------------------- hot path
static int eval_impl(const sunsky_emitter* e, sunsky_vec3_in w, const float* lam, int nlam, size_t lstride,
                     const uint8_t* active, size_t n, float* out, size_t ostride, void* stream, float sign) {
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (n == 0) return SUNSKY_OK;
    if (!w.x || !w.y || !w.z || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / output pointer");
    const bool spec = e->kargs.variant == kSpectral;
    if (int rc = check_ray_planes(spec, lam, nlam, n)) return rc;
    if (int rc = check_ray_strides(spec, nlam, lstride, ostride, n)) return rc;
    return guarded([&] {
        Launcher lc(e, stream);
        const bool dir = sign > 0.f;   // eval_direction: wo = d
        if (!spec) {
            const size_t n4 = vec4_count(n, {w.x, w.y, w.z, out}, {ostride}, active);
            vec4_then_tail(n, n4, [&](size_t off, size_t cnt, bool vec) {
                const float *x = w.x + off, *y = w.y + off, *z = w.z + off;
                const uint8_t* a = active ? active + off : nullptr;
                float* o = out + off;
                void* args[] = {&lc.K, &x, &y, &z, &a, &cnt, &o, &ostride, &sign};
                lc.run(vec ? K_EVAL_RGB_V4 : K_EVAL_RGB_V1, cnt, args, dir);
            });
        } else {
            // the wavelength planes too; either stride matters only when there is a second plane
            // (check_ray_strides): an odd stride next to a single plane keeps the vector kernels
            const size_t n4 = vec4_count(n, {w.x, w.y, w.z, out, lam}, {nlam == 1 ? 0 : ostride, nlam == 1 ? 0 : lstride},
                                         active);
            int nl = nlam;
            vec4_then_tail(n, n4, [&](size_t off, size_t cnt, bool vec) {
                const float *x = w.x + off, *y = w.y + off, *z = w.z + off, *l = lam + off;
                const uint8_t* a = active ? active + off : nullptr;
                float* o = out + off;
                void* args[] = {&lc.K, &x, &y, &z, &l, &lstride, &nl, &a, &cnt, &o, &ostride, &sign};
                // Mitsuba's Spectrum<Float, 4>: the kernel with the count compiled in
                lc.run(!vec ? K_EVAL_SPEC_RAYS_V1 : nlam == 4 ? K_EVAL_SPEC_RAYS4_V4 : K_EVAL_SPEC_RAYS_V4, cnt, args,
                       dir);
            });
        }
    });
}

int sunsky_eval(const sunsky_emitter* e, sunsky_vec3_in wi, const float* lam, int nlam, size_t lstride,
                const uint8_t* active, size_t n, float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "eval");
    return eval_impl(e, wi, lam, nlam, lstride, active, n, out, ostride, stream, -1.f);
}

int sunsky_eval_direction(const sunsky_emitter* e, sunsky_vec3_in d, const float* lam, int nlam, size_t lstride,
                          const uint8_t* active, size_t n, float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "eval_direction");
    return eval_impl(e, d, lam, nlam, lstride, active, n, out, ostride, stream, 1.f);
}

int sunsky_eval_spectral_broadcast(const sunsky_emitter* e, sunsky_vec3_in w, const float* lam_host, int m,
                                   const uint8_t* active, size_t n, float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "eval_spectral_broadcast");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (e->kargs.variant != kSpectral) return fail(SUNSKY_ERROR_INVALID_VALUE, "broadcast eval needs a spectral emitter");
    if (!lam_host || m < 1 || m > kMaxBroadcastLambda)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "1..32 broadcast wavelengths required");
    if (n == 0) return SUNSKY_OK;
    if (!w.x || !w.y || !w.z || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / output pointer");
    if (m > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    LambdaSet L = make_lambda_set(lam_host, m);
    // The 11 model wavelengths 320:40:720 in order: compile-time channel kernel.
    bool nodes = m == kNbWavelengths;
    for (int k = 0; nodes && k < m; ++k) nodes = L.lo[k] == k && L.f[k] == 0.f;
    return guarded([&] {
        Launcher lc(e, stream);
        float sign = -1.f;
        // one wavelength: out_stride is unused (no second plane), whatever its value
        const size_t n4 = vec4_count(n, {w.x, w.y, w.z, out}, {m == 1 ? 0 : ostride}, active);
        vec4_then_tail(n, n4, [&](size_t off, size_t cnt, bool vec) {
            const float *x = w.x + off, *y = w.y + off, *z = w.z + off;
            const uint8_t* a = active ? active + off : nullptr;
            float* o = out + off;
            void* args[] = {&lc.K, &L, &x, &y, &z, &a, &cnt, &o, &ostride, &sign};
            lc.run(!vec ? K_EVAL_SPEC_BCAST_V1 : nodes ? K_EVAL_SPEC_NODES_V4 : K_EVAL_SPEC_BCAST_V4, cnt, args);
        });
    });
}

int sunsky_sample_direction(const sunsky_emitter* e, const float* ux, const float* uy, sunsky_vec3_in it_p,
                            const float* lam, int nlam, size_t lstride, const uint8_t* active, size_t n,
                            sunsky_vec3_out ds_d, float* ds_pdf, float* ds_dist, sunsky_vec3_out ds_p,
                            float* weight, size_t wstride, void* stream) {
    SUNSKY_PHASE("EndpointSampleDirection", "sample_direction");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (n == 0) return SUNSKY_OK;
    const bool spec = e->kargs.variant == kSpectral;
    if (!ux || !uy || !ds_d.x || !ds_d.y || !ds_d.z || !ds_pdf || !weight)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null sample / output pointer");
    if (spec && (!lam || nlam < 1 || nlam > kMaxLambdaPerRay))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "spectral sample_direction needs 1..16 wavelength planes");
    if (wstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "weight_stride < n");
    if (int rc = check_optional_vec3(it_p, "it_p")) return rc;
    if (int rc = check_optional_vec3(ds_p, "ds_p")) return rc;
    return guarded([&] {
        Launcher lc(e, stream);
        int nl = spec ? nlam : 0;
        void* args[] = {&lc.K, &ux, &uy, (void*)&it_p.x, (void*)&it_p.y, (void*)&it_p.z, &lam, &lstride, &nl, &active, &n,
                        &ds_d.x, &ds_d.y, &ds_d.z, &ds_pdf, &ds_dist, &ds_p.x, &ds_p.y, &ds_p.z, &weight, &wstride};
        // the common call (no it.p, ds.dist, ds.p or mask) takes the kernel with those
        // paths compiled out: same results, no SGPR spills (sampling)
        const bool lean = !it_p.x && !ds_dist && !ds_p.x && !active;
        // SUNSKY_AMD_UNSORTED_SAMPLING=1: the unsorted LEAN kernels (A/B timing and the bitwise
        // sorted-vs-unsorted tests); read per call so a test can switch it
        const bool unsorted = unsorted_sampling();
        // SUNSKY_AMD_SORTED_GENERAL_SAMPLING=1: the masked general RGB call through the wave-sorted
        // kernel (10 % slower than the unsorted one; bitwise tests only)
        const bool sorted_general = env_switch("SUNSKY_AMD_SORTED_GENERAL_SAMPLING") && !unsorted;
        // spectral at Mitsuba's 4 wavelengths per sample: the wave-sorted kernel, LEAN or (no mask)
        // with ds.dist / ds.p from it.p read at the store stage.  RGB
        // without a mask (Mitsuba's DirectionSample call: it.p in, ds.dist / ds.p out) takes the
        // LEAN windows with each window's it.p loaded with its u, one window ahead (kSortPos); with
        // a mask, the unsorted general kernel.
        const KernelId k = spec ? (lean ? (nlam == 4 && !unsorted ? K_SAMPLE_DIRECTION_SPEC_LEAN4_SORTED
                                                                  : K_SAMPLE_DIRECTION_SPEC_LEAN)
                                        : (nlam == 4 && !active && !unsorted) ? K_SAMPLE_DIRECTION_SPEC_POS_SORTED
                                                                              : K_SAMPLE_DIRECTION_SPEC)
                                : (lean ? (unsorted ? K_SAMPLE_DIRECTION_RGB_LEAN_PLAIN : K_SAMPLE_DIRECTION_RGB_LEAN)
                                        : sorted_general ? K_SAMPLE_DIRECTION_RGB_FULL_SORTED
                                        : (!active && !unsorted) ? K_SAMPLE_DIRECTION_RGB_POS_SORTED
                                                                 : K_SAMPLE_DIRECTION_RGB);
        lc.run(k, n, args);
    });
}

int sunsky_pdf_direction(const sunsky_emitter* e, sunsky_vec3_in d, const uint8_t* active, size_t n, float* pdf,
                         void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "pdf_direction");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (n == 0) return SUNSKY_OK;
    if (!d.x || !d.y || !d.z || !pdf) return fail(SUNSKY_ERROR_INVALID_VALUE, "null direction / output pointer");
    return guarded([&] {
        Launcher lc(e, stream);
        const size_t n4 = vec4_count(n, {d.x, d.y, d.z, pdf}, {}, active);
        vec4_then_tail(n, n4, [&](size_t off, size_t cnt, bool vec) {
            const float *x = d.x + off, *y = d.y + off, *z = d.z + off;
            const uint8_t* a = active ? active + off : nullptr;
            float* p = pdf + off;
            void* args[] = {&lc.K, &x, &y, &z, &a, &cnt, &p};
            lc.run(vec ? K_PDF_DIRECTION_V4 : K_PDF_DIRECTION_V1, cnt, args);
        });
    });
}

int sunsky_sample_ray(const sunsky_emitter* e, const float* wls, const float* s2x, const float* s2y,
                      const float* s3x, const float* s3y, const uint8_t* active, size_t n, sunsky_vec3_out o,
                      sunsky_vec3_out d, float* lam, size_t lstride, float* weight, size_t wstride, void* stream) {
    SUNSKY_PHASE("EndpointSampleRay", "sample_ray");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (n == 0) return SUNSKY_OK;
    if (!s2x || !s2y || !s3x || !s3y || !o.x || !o.y || !o.z || !d.x || !d.y || !d.z || !lam || !weight)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null sample / output pointer");
    if (e->kargs.variant == kSpectral && !wls) return fail(SUNSKY_ERROR_INVALID_VALUE, "null wavelength sample");
    if (lstride < n || wstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "stride < n");
    return guarded([&] {
        Launcher lc(e, stream);
        void* args[] = {&lc.K, &wls, &s2x, &s2y, &s3x, &s3y, &active, &n, &o.x, &o.y, &o.z,
                        &d.x, &d.y, &d.z, &lam, &lstride, &weight, &wstride};
        // RGB without a mask: the wave-sorted kernel (one wave per window of 4 x 64 rays);
        // SUNSKY_AMD_UNSORTED_SAMPLING=1 keeps the unsorted one (A/B, the bitwise test)
        const bool unsorted = unsorted_sampling();
        const KernelId k = e->kargs.variant == kSpectral ? K_SAMPLE_RAY_SPEC
                           : (!active && !unsorted) ? K_SAMPLE_RAY_RGB_SORTED : K_SAMPLE_RAY_RGB;
        lc.run(k, n, args);
    });
}

int sunsky_sample_wavelengths(const sunsky_emitter* e, sunsky_vec3_in w, const float* sample, const uint8_t* active,
                              size_t n, float* lam, size_t lstride, float* weight, size_t wstride, void* stream) {
    SUNSKY_PHASE("EndpointSampleRay", "sample_wavelengths");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (n == 0) return SUNSKY_OK;
    if (!w.x || !w.y || !w.z || !lam || !weight) return fail(SUNSKY_ERROR_INVALID_VALUE, "null pointer");
    if (e->kargs.variant == kSpectral && !sample) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sample");
    if (lstride < n || wstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "stride < n");
    return guarded([&] {
        Launcher lc(e, stream);
        void* args[] = {&lc.K, (void*)&w.x, (void*)&w.y, (void*)&w.z, &sample, &active, &n, &lam, &lstride, &weight, &wstride};
        lc.run(e->kargs.variant == kSpectral ? K_SAMPLE_WAVELENGTHS_SPEC : K_SAMPLE_WAVELENGTHS_RGB, n, args);
    });
}

int sunsky_eval_jvp(const sunsky_emitter* e, int param, const float* tangent, int tangent_count, sunsky_vec3_in wi,
                    const float* lam, int nlam, size_t lstride, const uint8_t* active, size_t n, float* out,
                    float* d_out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "eval_jvp");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (!tangent) return fail(SUNSKY_ERROR_INVALID_VALUE, "null tangent");
    const bool spec = e->kargs.variant == kSpectral;
    if (int rc = check_ray_planes(spec, lam, nlam, n)) return rc;
    if (n && (!wi.x || !wi.y || !wi.z || !out || !d_out))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / output pointer");
    if (int rc = check_ray_strides(spec, nlam, lstride, ostride, n)) return rc;
    return guarded([&] {
        std::vector<float> key(tangent, tangent + std::max(0, tangent_count));
        key.push_back((float)param);
        const bool stage = !e->d_jvp.get() || e->jvp_rev != e->rev || key != e->jvp_key;
        TangentStage ts;
        if (stage || n == 0) ts = e->model->tangent_stage(param, tangent, tangent_count);   // validates param / count
        if (n == 0) return;
        Launcher lc(e, stream);
        hipStream_t st = lc.s;
        e->ad.begin(st, 0);   // ordered after the previous AD call (which may read d_jvp), any stream
        if (stage) {   // the tangent tables, staged on the device (sunsky_stage_tangent)
            if (!e->d_jvp.get()) e->d_jvp.alloc(sunsky_emitter::kJvpFloats);
            TangentArgs A = e->tangent_args(e->d_jvp.get(), 1, kTanSunLocal, 0, kJvpSunOffset, sunsky_emitter::kJvpFloats);
            A.st[0] = ts;
            e->stage_tangent(A, st);
            e->jvp_key = key;
            e->jvp_rev = e->rev;
        }
        const float* jvp = e->d_jvp.get();
        const float *x = wi.x, *y = wi.y, *z = wi.z;
        float sign = -1.f;
        if (!spec) {
            void* args[] = {&lc.K, &jvp, &x, &y, &z, &active, &n, &out, &d_out, &ostride, &sign};
            lc.run(K_EVAL_JVP_RGB, n, args);
        } else {
            int nl = nlam;
            void* args[] = {&lc.K, &jvp, &x, &y, &z, &lam, &lstride, &nl, &active, &n, &out, &d_out, &ostride, &sign};
            lc.run(K_EVAL_JVP_SPEC, n, args);
        }
        e->ad.end(st);
    });
}

int sunsky_emitter_tangent_tables(const sunsky_emitter* e, int param, const float* tangent, int tangent_count,
                                  int on_device, float* out, size_t cap, size_t* count) {
    if (!e || !count) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    if (!tangent) return fail(SUNSKY_ERROR_INVALID_VALUE, "null tangent");
    return guarded([&] {
        e->sync_host();
        const int total = sunsky_emitter::kJvpFloats;
        static_assert(sunsky_emitter::kJvpFloats == SUNSKY_TANGENT_FLOATS, "tangent buffer layout");
        std::vector<float> v(total, 0.f);
        if (on_device) {
            e->require_device();
            DeviceScope g(e->device);
            DeviceBuffer<float> d;
            d.alloc(total);
            TangentArgs A = e->tangent_args(d.get(), 1, kTanSunLocal, 0, kJvpSunOffset, total);
            A.st[0] = e->model->tangent_stage(param, tangent, tangent_count);
            e->stage_tangent(A, nullptr);
            hip_check(hipMemcpy(v.data(), d.get(), sizeof(float) * total, hipMemcpyDeviceToHost), "hipMemcpy");
        } else {
            const EvalTangent t = e->model->eval_tangent(param, tangent, tangent_count);
            std::memcpy(v.data(), t.dsky.data(), sizeof(float) * t.dsky.size());
            std::memcpy(v.data() + kTanSunLocal, t.dsun_local, 3 * sizeof(float));
            std::memcpy(v.data() + kJvpSunOffset, t.dsun.data(), sizeof(float) * t.dsun.size());
        }
        *count = v.size();
        if (out) std::memcpy(out, v.data(), sizeof(float) * std::min(cap, v.size()));
    });
}

int sunsky_eval_vjp(const sunsky_emitter* e, sunsky_vec3_in wi, const float* lam, int nlam, size_t lstride,
                    const uint8_t* active, size_t n, const float* d_out, size_t ostride, float* grad, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "eval_vjp");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (!grad) return fail(SUNSKY_ERROR_INVALID_VALUE, "null gradient buffer");
    const bool spec = e->kargs.variant == kSpectral;
    if (n == 0) return SUNSKY_OK;
    if (int rc = check_ray_planes(spec, lam, nlam, n)) return rc;
    if (!wi.x || !wi.y || !wi.z || !d_out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / cotangent pointer");
    if (int rc = check_ray_strides(spec, nlam, lstride, ostride, n)) return rc;
    return guarded([&] {
        Launcher lc(e, stream);
        // basis tangents: turbidity, albedo (all channels at once: channel c's tables depend on
        // albedo[c] only, so the all-ones tangent is the diagonal), sun_direction x / y / z
        const SunskyModel& M = *e->model;
        const int nch = M.nch();
        // the table's cap as it stands (untuned): the partials are sized by the grid
        const KernelId kernel = spec ? K_EVAL_VJP_SPEC : K_EVAL_VJP_RGB;
        const unsigned grid = grid_for(e->mod, kernel, n, /*tunable=*/false);
        hipStream_t st = lc.s;
        const bool stage = !e->d_vjp.get() || e->vjp_rev != e->rev;
        // ordered after the previous AD call (d_vjp / partials readers), any stream; 16 partials per workgroup
        float* partials = e->ad.begin(st, (size_t)16 * grid);
        if (stage) {   // the 5 basis tangents, staged on the device (sunsky_stage_tangent)
            if (!e->d_vjp.get()) e->d_vjp.alloc(sunsky_emitter::kVjpFloats);
            const int nb = M.active_record() ? 2 : kVjpBases;   // sun_direction is not exposed in time mode
            TangentArgs A = e->tangent_args(e->d_vjp.get(), nb, kVjpSunLocal, 2, kVjpSunOffset, sunsky_emitter::kVjpFloats);
            const float one = 1.f;
            A.st[0] = M.tangent_stage(kJvpTurbidity, &one, 1);
            std::vector<float> ones(nch, 1.f);
            A.st[1] = M.tangent_stage(kJvpAlbedo, ones.data(), nch);
            for (int k = 0; k + 2 < nb; ++k) {
                float axis[3] = {0.f, 0.f, 0.f};
                axis[k] = 1.f;
                A.st[2 + k] = M.tangent_stage(kJvpSunDirection, axis, 3);
            }
            if (nb == kVjpBases) {
                // the sky tables of sun axis k are d eta_k times those of a unit elevation
                // tangent: basis 2 holds the latter and the kernels scale by d eta_k
                // (kVjpSunEta), one sky tangent per channel for the 3 axes instead of 3
                A.eta_off = kVjpSunEta;
                A.st[2].dx = A.st[2].dx_per_eta;
                A.nsky = 3;   // the sky blocks of bases 3 and 4 are never read: written 0, not staged
            }
            e->stage_tangent(A, st);
            e->vjp_rev = e->rev;
        }
        const float* vjp = e->d_vjp.get();
        const float *x = wi.x, *y = wi.y, *z = wi.z;
        float sign = -1.f;
        if (!spec) {
            void* args[] = {&lc.K, &vjp, &x, &y, &z, &active, &n, &d_out, &ostride, &sign, &partials};
            lc.launch(kernel, grid, kBlock, args);
        } else {
            int nl = nlam;
            void* args[] = {&lc.K, &vjp, &x, &y, &z, &lam, &lstride, &nl, &active, &n, &d_out, &ostride, &sign, &partials};
            lc.launch(kernel, grid, kBlock, args);
        }
        unsigned nb = grid;
        void* rargs[] = {&partials, &nb, &grad};
        lc.launch(K_GRAD_REDUCE, 1, kBlock, rargs);
        e->ad.end(st);
    });
}

// d eval / d wi: argument checks shared by the two calls (sunsky_eval_jvp's rules)
static int dir_ad_check(const sunsky_emitter* e, sunsky_vec3_in wi, const float* lam, int nlam, size_t lstride,
                        size_t n, bool planes_ok, size_t ostride) {
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    const bool spec = e->kargs.variant == kSpectral;
    if (int rc = check_ray_planes(spec, lam, nlam, n)) return rc;
    if (n && (!wi.x || !wi.y || !wi.z || !planes_ok))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / tangent / output pointer");
    return check_ray_strides(spec, nlam, lstride, ostride, n);
}

int sunsky_eval_jvp_dir(const sunsky_emitter* e, sunsky_vec3_in wi, sunsky_vec3_in d_wi, const float* lam, int nlam,
                        size_t lstride, const uint8_t* active, size_t n, float* out, float* d_out, size_t ostride,
                        void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "eval_jvp_dir");
    if (int rc = dir_ad_check(e, wi, lam, nlam, lstride, n, d_wi.x && d_wi.y && d_wi.z && out && d_out, ostride))
        return rc;
    if (n == 0) return SUNSKY_OK;
    return guarded([&] {
        Launcher lc(e, stream);
        const float *x = wi.x, *y = wi.y, *z = wi.z, *dx = d_wi.x, *dy = d_wi.y, *dz = d_wi.z;
        float sign = -1.f;
        if (e->kargs.variant != kSpectral) {
            void* args[] = {&lc.K, &x, &y, &z, &dx, &dy, &dz, &active, &n, &out, &d_out, &ostride, &sign};
            lc.run(K_EVAL_JVP_DIR_RGB, n, args);
        } else {
            int nl = nlam;
            void* args[] = {&lc.K, &x, &y, &z, &dx, &dy, &dz, &lam, &lstride, &nl, &active, &n, &out, &d_out, &ostride, &sign};
            lc.run(K_EVAL_JVP_DIR_SPEC, n, args);
        }
    });
}

int sunsky_eval_vjp_dir(const sunsky_emitter* e, sunsky_vec3_in wi, const float* lam, int nlam, size_t lstride,
                        const uint8_t* active, size_t n, const float* d_out, size_t ostride, sunsky_vec3_out grad_wi,
                        void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "eval_vjp_dir");
    if (int rc = dir_ad_check(e, wi, lam, nlam, lstride, n, d_out && grad_wi.x && grad_wi.y && grad_wi.z, ostride))
        return rc;
    if (n == 0) return SUNSKY_OK;
    return guarded([&] {
        Launcher lc(e, stream);
        const float *x = wi.x, *y = wi.y, *z = wi.z;
        float *gx = grad_wi.x, *gy = grad_wi.y, *gz = grad_wi.z;
        float sign = -1.f;
        if (e->kargs.variant != kSpectral) {
            void* args[] = {&lc.K, &x, &y, &z, &active, &n, &d_out, &ostride, &gx, &gy, &gz, &sign};
            lc.run(K_EVAL_VJP_DIR_RGB, n, args);
        } else {
            int nl = nlam;
            void* args[] = {&lc.K, &x, &y, &z, &lam, &lstride, &nl, &active, &n, &d_out, &ostride, &gx, &gy, &gz, &sign};
            lc.run(K_EVAL_VJP_DIR_SPEC, n, args);
        }
    });
}

int sunsky_bake_latlong(const sunsky_emitter* e, int width, int height, float theta0, float theta1, float phi0,
                        float phi1, const float* lam_host, int m, float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "bake_latlong");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    const bool spec = e->kargs.variant == kSpectral;
    LatLong G;
    if (int rc = check_bake(spec, width, height, theta0, theta1, phi0, phi1, lam_host, m, out, ostride, &G)) return rc;
    const size_t n = (size_t)width * (size_t)height;
    return guarded([&] {
        Launcher lc(e, stream);
        // the angle tables are per emitter: order this bake after the previous one (any
        // stream), so a bake on another stream cannot rewrite them under a running kernel
        float* tab = e->bake.begin(lc.s, 2 * (size_t)width + 2 * (size_t)height);
        G.tab = tab;
        {
            void* targs[] = {&G, &tab};
            lc.launch(K_LATLONG_TABLES, (unsigned)((std::max(width, height) + kBlock - 1) / kBlock), kBlock, targs);
        }
        if (!spec) {
            // 4 pixels of a row per thread, each row rounded up
            void* args[] = {&lc.K, &G, &out, &ostride};
            lc.run(K_BAKE_RGB, (size_t)((width + 3) / 4) * height, args);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&lc.K, &G, &L, &out, &ostride};
            lc.run(K_BAKE_SPEC, n, args);
        }
        e->bake.end(lc.s);
    });
}

int sunsky_direct_diffuse(const sunsky_emitter* e, sunsky_vec3_in nrm, const float* rho, const float* lam, int nlam,
                          size_t lstride, uint32_t seed, uint32_t spp, const uint8_t* vis, size_t vstride, size_t n,
                          float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("SamplingIntegratorSample", "direct_diffuse");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (n == 0) return SUNSKY_OK;
    const bool spec = e->kargs.variant == kSpectral;
    if (!nrm.x || !nrm.y || !nrm.z || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal / output pointer");
    if (spp < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "spp must be >= 1");
    if (n > 0xffffffffull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 points (the sampler's lane index is 32-bit)");
    if (spec && (!lam || nlam < 1 || nlam > 4))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "spectral direct lighting needs 1..4 wavelength planes");
    if (!spec && (lam || nlam)) return fail(SUNSKY_ERROR_INVALID_VALUE, "RGB direct lighting takes no wavelengths");
    if (ostride < n || (spec && lstride < n)) return fail(SUNSKY_ERROR_INVALID_VALUE, "stride < n");
    if (vis && vstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "vis_stride < n");
    return guarded([&] {
        Launcher lc(e, stream);
        int nl = spec ? nlam : 0;
        void* args[] = {&lc.K, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &rho, &lam, &lstride, &nl, &seed, &spp, &vis,
                        &vstride, &n, &out, &ostride};
        lc.run(spec ? K_DIRECT_DIFFUSE_SPEC : K_DIRECT_DIFFUSE_RGB, n, args);
    });
}

int sunsky_direct_diffuse_rays(const sunsky_emitter* e, sunsky_vec3_in nrm, uint32_t seed, uint32_t spp, size_t n,
                               sunsky_vec3_out em, sunsky_vec3_out bs, size_t rstride, void* stream) {
    SUNSKY_PHASE("SamplingIntegratorSample", "direct_diffuse_rays");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (n == 0) return SUNSKY_OK;
    if (!nrm.x || !nrm.y || !nrm.z) return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal pointer");
    if (!em.x || !em.y || !em.z || !bs.x || !bs.y || !bs.z) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray pointer");
    if (spp < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "spp must be >= 1");
    if (n > 0xffffffffull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 points (the sampler's lane index is 32-bit)");
    if (rstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "ray_stride < n");
    return guarded([&] {
        Launcher lc(e, stream);
        void* args[] = {&lc.K, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &seed, &spp, &n, &em.x, &em.y, &em.z,
                        &bs.x, &bs.y, &bs.z, &rstride};
        lc.run(K_DIRECT_DIFFUSE_RAYS, n, args);
    });
}

// The rough conductor of the glossy caller (ConductorArgs, sunsky_kernel_args.h)
static int conductor_args(const sunsky_emitter* e, int distribution, float alpha_u, float alpha_v, const float* eta,
                          const float* k, ConductorArgs* c) {
    if (distribution != SUNSKY_MICROFACET_BECKMANN && distribution != SUNSKY_MICROFACET_GGX)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "distribution must be SUNSKY_MICROFACET_BECKMANN or _GGX");
    if (!(alpha_u > 0.f) || !(alpha_v > 0.f) || std::isinf(alpha_u) || std::isinf(alpha_v))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "alpha (alpha_u, alpha_v) must be finite and > 0");
    if (!eta || !k) return fail(SUNSKY_ERROR_INVALID_VALUE, "null eta / k");
    std::memset(c, 0, sizeof(*c));
    c->type = distribution;
    // microfacet.h clamps alpha_u, alpha_v to 1e-4 (MicrofacetDistribution::configure, :424-428)
    c->alpha_u = std::max(alpha_u, 1e-4f);
    c->alpha_v = std::max(alpha_v, 1e-4f);
    const int nc = e->kargs.variant == kSpectral ? 1 : 3;
    for (int i = 0; i < nc; ++i) { c->eta[i] = eta[i]; c->k[i] = k[i]; }
    return SUNSKY_OK;
}

static int direct_conductor_impl(const sunsky_emitter* e, sunsky_vec3_in nrm, sunsky_vec3_in wi, int distribution,
                                 float alpha_u, float alpha_v, const float* eta, const float* k, const float* lam,
                                 int nlam, size_t lstride, uint32_t seed, uint32_t spp, const uint8_t* vis,
                                 size_t vstride, size_t n, float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("SamplingIntegratorSample", "direct_conductor");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    ConductorArgs C;
    int rc = conductor_args(e, distribution, alpha_u, alpha_v, eta, k, &C);
    if (rc != SUNSKY_OK) return rc;
    if (n == 0) return SUNSKY_OK;
    const bool spec = e->kargs.variant == kSpectral;
    if (!nrm.x || !nrm.y || !nrm.z || !wi.x || !wi.y || !wi.z || !out)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal / view direction / output pointer");
    if (spp < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "spp must be >= 1");
    if (n > 0xffffffffull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 points (the sampler's lane index is 32-bit)");
    if (spec && (!lam || nlam < 1 || nlam > 4))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "spectral direct lighting needs 1..4 wavelength planes");
    if (!spec && (lam || nlam)) return fail(SUNSKY_ERROR_INVALID_VALUE, "RGB direct lighting takes no wavelengths");
    if (ostride < n || (spec && lstride < n)) return fail(SUNSKY_ERROR_INVALID_VALUE, "stride < n");
    if (vis && vstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "vis_stride < n");
    return guarded([&] {
        Launcher lc(e, stream);
        int nl = spec ? nlam : 0;
        void* args[] = {&lc.K, &C, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, (void*)&wi.x, (void*)&wi.y, (void*)&wi.z,
                        &lam, &lstride, &nl, &seed, &spp, &vis, &vstride, &n, &out, &ostride};
        lc.run(spec ? K_DIRECT_CONDUCTOR_SPEC : K_DIRECT_CONDUCTOR_RGB, n, args);
    });
}

static int direct_conductor_rays_impl(const sunsky_emitter* e, sunsky_vec3_in nrm, sunsky_vec3_in wi,
                                      int distribution, float alpha_u, float alpha_v, const float* eta, const float* k,
                                      uint32_t seed, uint32_t spp, size_t n, sunsky_vec3_out em, sunsky_vec3_out bs,
                                      float* bw, size_t rstride, void* stream) {
    SUNSKY_PHASE("SamplingIntegratorSample", "direct_conductor_rays");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (bw && (!eta || !k)) return fail(SUNSKY_ERROR_INVALID_VALUE, "the BSDF weights need eta / k");
    const float one[3] = {1.f, 1.f, 1.f};
    ConductorArgs C;
    // the directions do not depend on eta / k; the weights do
    int rc = conductor_args(e, distribution, alpha_u, alpha_v, bw ? eta : one, bw ? k : one, &C);
    if (rc != SUNSKY_OK) return rc;
    int nw = e->kargs.variant == kSpectral ? 1 : 3;
    if (n == 0) return SUNSKY_OK;
    if (!nrm.x || !nrm.y || !nrm.z || !wi.x || !wi.y || !wi.z)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null normal / view direction pointer");
    if (!em.x || !em.y || !em.z || !bs.x || !bs.y || !bs.z) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray pointer");
    if (spp < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "spp must be >= 1");
    if (n > 0xffffffffull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 points (the sampler's lane index is 32-bit)");
    if (rstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "ray_stride < n");
    return guarded([&] {
        Launcher lc(e, stream);
        void* args[] = {&lc.K, &C, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, (void*)&wi.x, (void*)&wi.y, (void*)&wi.z,
                        &seed, &spp, &n, &em.x, &em.y, &em.z, &bs.x, &bs.y, &bs.z, &rstride, &bw, &nw};
        lc.run(K_DIRECT_CONDUCTOR_RAYS, n, args);
    });
}

int sunsky_direct_conductor(const sunsky_emitter* e, sunsky_vec3_in nrm, sunsky_vec3_in wi, int distribution,
                            float alpha, const float* eta, const float* k, const float* lam, int nlam, size_t lstride,
                            uint32_t seed, uint32_t spp, const uint8_t* vis, size_t vstride, size_t n, float* out,
                            size_t ostride, void* stream) {
    return direct_conductor_impl(e, nrm, wi, distribution, alpha, alpha, eta, k, lam, nlam, lstride, seed, spp, vis,
                                 vstride, n, out, ostride, stream);
}

int sunsky_direct_conductor_aniso(const sunsky_emitter* e, sunsky_vec3_in nrm, sunsky_vec3_in wi, int distribution,
                                  float alpha_u, float alpha_v, const float* eta, const float* k, const float* lam,
                                  int nlam, size_t lstride, uint32_t seed, uint32_t spp, const uint8_t* vis,
                                  size_t vstride, size_t n, float* out, size_t ostride, void* stream) {
    return direct_conductor_impl(e, nrm, wi, distribution, alpha_u, alpha_v, eta, k, lam, nlam, lstride, seed, spp,
                                 vis, vstride, n, out, ostride, stream);
}

int sunsky_direct_conductor_rays(const sunsky_emitter* e, sunsky_vec3_in nrm, sunsky_vec3_in wi, int distribution,
                                 float alpha, const float* eta, const float* k, uint32_t seed, uint32_t spp, size_t n,
                                 sunsky_vec3_out em, sunsky_vec3_out bs, float* bw, size_t rstride, void* stream) {
    return direct_conductor_rays_impl(e, nrm, wi, distribution, alpha, alpha, eta, k, seed, spp, n, em, bs, bw, rstride,
                                      stream);
}

int sunsky_direct_conductor_rays_aniso(const sunsky_emitter* e, sunsky_vec3_in nrm, sunsky_vec3_in wi,
                                       int distribution, float alpha_u, float alpha_v, const float* eta,
                                       const float* k, uint32_t seed, uint32_t spp, size_t n, sunsky_vec3_out em,
                                       sunsky_vec3_out bs, float* bw, size_t rstride, void* stream) {
    return direct_conductor_rays_impl(e, nrm, wi, distribution, alpha_u, alpha_v, eta, k, seed, spp, n, em, bs, bw,
                                      rstride, stream);
}

int sunsky_sample_position(const sunsky_emitter* e) {
    (void)e;
    return fail(SUNSKY_ERROR_NOT_IMPLEMENTED, "sample_position");
}

}  // extern "C"
