// sunsky_launch.h -- what the C-ABI entry points (sunsky_capi_*.cpp) launch with: the kernel
// table and the per-device module, grid sizing, owned device memory, the launcher of a batch
// entry point, the ordered scratch buffer and the argument checks several entry points share.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sunsky_amd.h"
#include "sunsky_errors.h"
#include "sunsky_kernel_args.h"
#include "sunsky_model.h"
#include "sunsky_profiler.h"
#include "sunsky_types.h"

namespace sunsky {
namespace capi {

std::string default_pack_path();   // SUNSKY_AMD_DATASET, else the pack beside the library

// ---------------------------------------------------------------- kernels
// The sampling kernels are instantiated per variant (RGB / spectral) so each
// carries only its own tables and registers.
//
// The kernel table, one row per kernel: X(id, name, workgroups per CU, dir, per, forms).
//  * name: the code objects export name_fast and name_ref (FOUR forms), or name (PLAIN).
//  * workgroups per CU: the cap of the grid-stride launches, sized to fill every CU several
//    times over (cdna_hip_programming.md Guideline 11).  From the tools/kbench.cpp sweep on
//    MI355X (profiles/r01_v2_kbench_grid_sweep.log): RGB eval 64 (60.4 us vs 64.9 us at 16
//    for 16M directions), spectral 64, sampling 64 (profiles/r01_v5_kbench.log,
//    r01_v7_tune.log); sample_ray 32, from the sweep over 8/16/32/64
//    (profiles/r03_v18_kbench_grid_ray_wavelengths.log); 16 where no sweep is recorded.  The
//    sequence kernels (one ray per lane, bound by VALU issue, not memory) take 64: one step per
//    lane up to 4M rays, where the cap only bounds the grid.  The sequence VJP kernels take 16:
//    every wave owns a row of the reduction workspace (sunsky_kernel_args.h), so fewer, longer
//    workgroups keep the workspace and the reduce pass small.  The AD kernels of eval take the
//    cap of the eval kernel they differentiate (64); eval_vjp takes 6 (the RGB kernel holds 3
//    workgroups per CU at a time, 134 VGPRs): few per-block partials, so the one-workgroup
//    reduce after it stays short (16384 partials took 0.3 ms).  0: the kernel is launched on
//    a grid its call site fixes (staging, tables, reduces), never through grid_for.
//  * dir: the eval kernels are instantiated twice: eval(si) negates wi at compile time,
//    eval_direction(ds) uses ds.d as is (name_dir_fast, name_dir_ref).
//  * per: samples per work item: 4 consecutive directions per lane in the VEC = 4 kernels
//    (their batches are multiples of 4); in the wave-sorted kernels one wave takes a window
//    of 4 (RGB) or 3 (spectral) x 64 samples.
//  * forms: FOUR: the kernel exists in {general, identity to_world} x {_fast, _ref}; PLAIN: in
//    one form, loaded from the general code object (to_world and precision do not enter it).
#define SUNSKY_KERNELS(X)                                                                          \
    X(EVAL_RGB_V4, "sunsky_eval_rgb_v4", 64, true, 4, FOUR)                                        \
    X(EVAL_RGB_V1, "sunsky_eval_rgb_v1", 64, true, 1, FOUR)                                        \
    X(EVAL_SPEC_BCAST_V4, "sunsky_eval_spec_bcast_v4", 64, false, 4, FOUR)                         \
    X(EVAL_SPEC_BCAST_V1, "sunsky_eval_spec_bcast_v1", 64, false, 1, FOUR)                         \
    X(EVAL_SPEC_NODES_V4, "sunsky_eval_spec_nodes_v4", 64, false, 4, FOUR)                         \
    X(EVAL_SPEC_RAYS_V4, "sunsky_eval_spec_rays_v4", 64, true, 4, FOUR)                            \
    X(EVAL_SPEC_RAYS_V1, "sunsky_eval_spec_rays_v1", 64, true, 1, FOUR)                            \
    X(EVAL_SPEC_RAYS4_V4, "sunsky_eval_spec_rays4_v4", 64, true, 4, FOUR)                          \
    X(PDF_DIRECTION_V4, "sunsky_pdf_direction_v4", 64, false, 4, FOUR)                             \
    X(PDF_DIRECTION_V1, "sunsky_pdf_direction_v1", 64, false, 1, FOUR)                             \
    X(SAMPLE_DIRECTION_RGB, "sunsky_sample_direction_rgb", 64, false, 1, FOUR)                     \
    X(SAMPLE_DIRECTION_RGB_LEAN, "sunsky_sample_direction_rgb_lean", 64, false, 4, FOUR)           \
    X(SAMPLE_DIRECTION_RGB_LEAN_PLAIN, "sunsky_sample_direction_rgb_lean_plain", 64, false, 1, FOUR) \
    X(SAMPLE_DIRECTION_RGB_FULL_SORTED, "sunsky_sample_direction_rgb_full_sorted", 64, false, 4, FOUR) \
    X(SAMPLE_DIRECTION_RGB_POS_SORTED, "sunsky_sample_direction_rgb_pos_sorted", 64, false, 4, FOUR) \
    X(SAMPLE_DIRECTION_SPEC, "sunsky_sample_direction_spec", 64, false, 1, FOUR)                   \
    X(SAMPLE_DIRECTION_SPEC_LEAN, "sunsky_sample_direction_spec_lean", 64, false, 1, FOUR)         \
    X(SAMPLE_DIRECTION_SPEC_LEAN4_SORTED, "sunsky_sample_direction_spec_lean4_sorted", 64, false, 3, FOUR) \
    X(SAMPLE_DIRECTION_SPEC_POS_SORTED, "sunsky_sample_direction_spec_pos_sorted", 64, false, 3, FOUR) \
    X(SAMPLE_RAY_RGB, "sunsky_sample_ray_rgb", 32, false, 1, FOUR)                                 \
    X(SAMPLE_RAY_RGB_SORTED, "sunsky_sample_ray_rgb_sorted", 64, false, 4, FOUR)                   \
    X(SAMPLE_RAY_SPEC, "sunsky_sample_ray_spec", 32, false, 1, FOUR)                               \
    X(SAMPLE_WAVELENGTHS_RGB, "sunsky_sample_wavelengths_rgb", 16, false, 1, FOUR)                 \
    X(SAMPLE_WAVELENGTHS_SPEC, "sunsky_sample_wavelengths_spec", 64, false, 1, FOUR)               \
    X(BAKE_RGB, "sunsky_bake_latlong_rgb", 64, false, 1, FOUR)                                     \
    X(BAKE_SPEC, "sunsky_bake_latlong_spec", 64, false, 1, FOUR)                                   \
    X(DIRECT_DIFFUSE_RGB, "sunsky_direct_diffuse_rgb", 64, false, 1, FOUR)                         \
    X(DIRECT_DIFFUSE_SPEC, "sunsky_direct_diffuse_spec", 64, false, 1, FOUR)                       \
    X(DIRECT_DIFFUSE_RAYS, "sunsky_direct_diffuse_rays", 64, false, 1, FOUR)                       \
    X(DIRECT_CONDUCTOR_RGB, "sunsky_direct_conductor_rgb", 64, false, 1, FOUR)                     \
    X(DIRECT_CONDUCTOR_SPEC, "sunsky_direct_conductor_spec", 64, false, 1, FOUR)                   \
    X(DIRECT_CONDUCTOR_RAYS, "sunsky_direct_conductor_rays", 64, false, 1, FOUR)                   \
    X(SEQUENCE_EVAL_RGB, "sunsky_sequence_eval_rgb", 64, false, 1, FOUR)                           \
    X(SEQUENCE_EVAL_SPEC, "sunsky_sequence_eval_spec", 64, false, 1, FOUR)                         \
    X(SEQUENCE_BAKE_RGB, "sunsky_sequence_bake_rgb", 64, false, 1, FOUR)                           \
    X(SEQUENCE_BAKE_SPEC, "sunsky_sequence_bake_spec", 64, false, 1, FOUR)                         \
    X(SEQUENCE_SAMPLE_RGB, "sunsky_sequence_sample_rgb", 64, false, 1, FOUR)                       \
    X(SEQUENCE_SAMPLE_SPEC, "sunsky_sequence_sample_spec", 64, false, 1, FOUR)                     \
    X(SEQUENCE_PDF, "sunsky_sequence_pdf", 64, false, 1, FOUR)                                     \
    X(SEQUENCE_EVAL_VJP_RGB, "sunsky_sequence_eval_vjp_rgb", kSeqGradBlocksPerCu, false, 1, FOUR)  \
    X(SEQUENCE_EVAL_VJP_SPEC, "sunsky_sequence_eval_vjp_spec", kSeqGradBlocksPerCu, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_RGB, "sunsky_sequence_irradiance_rgb", 64, false, 2, FOUR)               \
    X(SEQUENCE_IRRADIANCE_SPEC, "sunsky_sequence_irradiance_spec", 64, false, 2, FOUR)             \
    X(SEQUENCE_IRRADIANCE_HORIZON_RGB, "sunsky_sequence_irradiance_horizon_rgb", 64, false, 2, FOUR) \
    X(SEQUENCE_IRRADIANCE_HORIZON_SPEC, "sunsky_sequence_irradiance_horizon_spec", 64, false, 2, FOUR) \
    X(SEQUENCE_IRRADIANCE_SERIES_RGB, "sunsky_sequence_irradiance_series_rgb", 64, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_SERIES_SPEC, "sunsky_sequence_irradiance_series_spec", 64, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_SERIES_HORIZON_RGB, "sunsky_sequence_irradiance_series_horizon_rgb", 64, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_SERIES_HORIZON_SPEC, "sunsky_sequence_irradiance_series_horizon_spec", 64, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_VJP_NORMAL_RGB, "sunsky_sequence_irradiance_vjp_normal_rgb", 64, false, 2, FOUR) \
    X(SEQUENCE_IRRADIANCE_VJP_NORMAL_SPEC, "sunsky_sequence_irradiance_vjp_normal_spec", 64, false, 2, FOUR) \
    X(SEQUENCE_IRRADIANCE_ADJOINT, "sunsky_sequence_irradiance_adjoint", kSeqIrrGradAdjointBlocksPerCu, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_GRAD_FOLD, "sunsky_sequence_irradiance_grad_fold", kSeqIrrGradFoldBlocksPerCu, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_HORIZON_VJP_NORMAL_RGB, "sunsky_sequence_irradiance_horizon_vjp_normal_rgb", 64, false, 2, FOUR) \
    X(SEQUENCE_IRRADIANCE_HORIZON_VJP_NORMAL_SPEC, "sunsky_sequence_irradiance_horizon_vjp_normal_spec", 64, false, 2, FOUR) \
    X(SEQUENCE_IRRADIANCE_HORIZON_VJP_PROFILE_RGB, "sunsky_sequence_irradiance_horizon_vjp_profile_rgb", 64, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_HORIZON_VJP_PROFILE_SPEC, "sunsky_sequence_irradiance_horizon_vjp_profile_spec", 64, false, 1, FOUR) \
    X(SEQUENCE_IRRADIANCE_HORIZON_ADJOINT, "sunsky_sequence_irradiance_horizon_adjoint", kSeqIrrGradAdjointBlocksPerCu, false, 1, FOUR) \
    X(DEBUG_SUN_SEGMENTS, "sunsky_debug_sun_segments", 16, false, 1, FOUR)                         \
    X(EVAL_JVP_RGB, "sunsky_eval_jvp_rgb", 64, false, 1, PLAIN)                                    \
    X(EVAL_JVP_SPEC, "sunsky_eval_jvp_spec", 64, false, 1, PLAIN)                                  \
    X(EVAL_VJP_RGB, "sunsky_eval_vjp_rgb", 6, false, 1, PLAIN)                                     \
    X(EVAL_VJP_SPEC, "sunsky_eval_vjp_spec", 6, false, 1, PLAIN)                                   \
    X(GRAD_REDUCE, "sunsky_grad_reduce", 0, false, 1, PLAIN)                                       \
    X(EVAL_JVP_DIR_RGB, "sunsky_eval_jvp_dir_rgb", 64, false, 1, PLAIN)                            \
    X(EVAL_JVP_DIR_SPEC, "sunsky_eval_jvp_dir_spec", 64, false, 1, PLAIN)                          \
    X(EVAL_VJP_DIR_RGB, "sunsky_eval_vjp_dir_rgb", 64, false, 1, PLAIN)                            \
    X(EVAL_VJP_DIR_SPEC, "sunsky_eval_vjp_dir_spec", 64, false, 1, PLAIN)                          \
    X(LATLONG_TABLES, "sunsky_latlong_tables", 0, false, 1, PLAIN)                                 \
    X(STAGE_RADIANCE, "sunsky_stage_radiance", 0, false, 1, PLAIN)                                 \
    X(STAGE_QUAD_POINTS, "sunsky_stage_quad_points", 0, false, 1, PLAIN)                           \
    X(STAGE_QUAD_FINISH, "sunsky_stage_quad_finish", 0, false, 1, PLAIN)                           \
    X(STAGE_TANGENT, "sunsky_stage_tangent", 0, false, 1, PLAIN)                                   \
    X(STAGE_SEQUENCE, "sunsky_stage_sequence", 0, false, 1, PLAIN)                                 \
    X(STAGE_SEQUENCE_GRAD, "sunsky_stage_sequence_grad", 0, false, 1, PLAIN)                       \
    X(SEQUENCE_TABLE, "sunsky_sequence_table", 64, false, 1, PLAIN)                                \
    X(SEQUENCE_SUNS, "sunsky_sequence_suns", 0, false, 1, PLAIN)                                   \
    X(SEQUENCE_GRAD_REDUCE, "sunsky_sequence_grad_reduce", 0, false, 1, PLAIN)                     \
    X(SEQUENCE_IRRADIANCE_TABLE, "sunsky_sequence_irradiance_table", 64, false, 1, PLAIN)          \
    X(SEQUENCE_IRRADIANCE_FLUX, "sunsky_sequence_irradiance_flux", 0, false, 1, PLAIN)               \
    X(SEQUENCE_IRRADIANCE_SERIES_TABLE, "sunsky_sequence_irradiance_series_table", 64, false, 1, PLAIN)

#define X(id, name, wg, dir, per, forms) K_##id,
enum KernelId { SUNSKY_KERNELS(X) K_COUNT };
#undef X
enum KernelForms { FOUR, PLAIN };
struct KernelInfo {
    const char* name;
    int blocks_per_cu;
    bool dir_form;
    int per_item;
    KernelForms forms;
};
#define X(id, name, wg, dir, per, forms) {name, wg, dir, per, forms},
constexpr KernelInfo kKernels[] = {SUNSKY_KERNELS(X)};
#undef X
static_assert(sizeof(kKernels) / sizeof(kKernels[0]) == K_COUNT, "one table row per KernelId");

struct DeviceModule {
    hipModule_t module = nullptr, module_ident = nullptr;
    // [identity to_world][precision][kernel]: [1] from sunsky_kernels_ident.hsaco.  A PLAIN
    // kernel's one function stands in all four places.
    hipFunction_t fn[2][2][K_COUNT] = {};
    hipFunction_t fn_dir[2][2][K_COUNT] = {};   // eval_direction forms (wo = +d) of the eval kernels
    int cu_count = 256;
};
DeviceModule* module_for_device(int dev);

// Workgroup sizes, beside kQuadBlock and kSeqGradReduceBlock (sunsky_kernel_args.h)
constexpr int kBlock = 256;
constexpr int kWaveBlock = 64;   // one wave per frame: sunsky_sequence_suns, sunsky_sequence_irradiance_flux

// Grid of a grid-stride launch of kernel k over `work_items`: one thread each, up to the
// table's workgroups per CU.  SUNSKY_AMD_BLOCKS_PER_CU overrides every kernel's (read once),
// except for the launches the override has never reached, which pass tunable = false:
// eval_vjp (its partials are sized by the grid) and the two sequence table kernels.
unsigned grid_for(const DeviceModule* m, KernelId k, size_t work_items, bool tunable = true);

// The one launch of the library: `grid` workgroups of `block` threads
void launch(hipFunction_t f, unsigned grid, unsigned block, hipStream_t stream, void** args, unsigned dyn_lds = 0);
// ... of a PLAIN kernel of the table
inline void launch(const DeviceModule* m, KernelId k, unsigned grid, unsigned block, hipStream_t stream, void** args) {
    launch(m->fn[0][0][k], grid, block, stream, args);
}

// Kernel k of code object `form` (1: identity to_world) and `precision` over n samples on
// stream s.  dir: the eval_direction form (wo = d) of an eval kernel.
void run_kernel(const DeviceModule* mod, int form, int precision, KernelId k, size_t n, void** args, hipStream_t s,
                bool dir = false);

// The VEC = 4 kernels move 16 bytes per lane and plane (4 mask bytes).  How many of a batch's
// n samples they can take: the multiple of 4 below n when every plane of `planes` is 16-byte
// aligned, every plane stride of `strides` a multiple of 4 and the mask 4-byte aligned, else 0.
size_t vec4_count(size_t n, std::initializer_list<const void*> planes, std::initializer_list<size_t> strides,
                  const uint8_t* active);

// part(offset, count, vec): the VEC = 4 body over [0, n4), then the VEC = 1 tail over [n4, n)
template <typename F>
void vec4_then_tail(size_t n, size_t n4, F&& part) {
    if (n4) part((size_t)0, n4, true);
    if (n4 < n) part(n4, n - n4, false);
}

// normalized_wavelengths / floor2int / lerp factor of eval, sunsky.cpp:326-332
LambdaSet make_lambda_set(const float* lam, int m);

// Makes a handle's device current for the scope of an entry point: every allocation, event
// and launch of an emitter or sequence happens on its own GPU whatever the caller's current
// device is.
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) {
        if (dev < 0) return;
        int cur = 0;
        hip_check(hipGetDevice(&cur), "hipGetDevice");
        if (cur != dev) {
            hip_check(hipSetDevice(dev), "hipSetDevice");
            prev = cur;
        }
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// ---------------------------------------------------------------- owned device memory
// n elements of T from hipMalloc, freed on destruction.  Move-only.  Views into a block
// (d_qx, d_sky_rad_ds, ...) stay plain pointers beside their owner.
template <typename T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept { *this = std::move(o); }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {   // the source frees what this held
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    void alloc(size_t n) {
        reset();
        hip_check(hipMalloc(&p_, sizeof(T) * n), "hipMalloc");
        n_ = n;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// n elements of T in pinned host memory
template <typename T>
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { if (p_) (void)hipHostFree(p_); }
    T* get() const { return p_; }
    void alloc(size_t n) { hip_check(hipHostMalloc((void**)&p_, sizeof(T) * n, hipHostMallocDefault), "hipHostMalloc"); }

private:
    T* p_ = nullptr;
};

// An ordering event (no timing), created on demand
class DeviceEvent {
public:
    DeviceEvent() = default;
    DeviceEvent(const DeviceEvent&) = delete;
    DeviceEvent& operator=(const DeviceEvent&) = delete;
    ~DeviceEvent() { if (e_) (void)hipEventDestroy(e_); }
    hipEvent_t get() const { return e_; }
    void create() { hip_check(hipEventCreateWithFlags(&e_, hipEventDisableTiming), "hipEventCreate"); }

private:
    hipEvent_t e_ = nullptr;
};

// How a handle that owns device memory is destroyed.  The handle declares this as its FIRST
// member and calls enter(device) from its destructor body.  The body runs before any member is
// destroyed and members are destroyed in reverse order of declaration, so every owner declared
// after this frees its memory with the handle's device current and after the drain; this
// member goes last and gives the caller's device back.
struct DrainOnDestroy {
    int prev = -1;
    void enter(int device) {
        if (device < 0) return;   // host-only handle: owns nothing on a device
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess) prev = cur;
        // a destroyed handle may still be read by launches in flight on any stream
        (void)hipDeviceSynchronize();
    }
    ~DrainOnDestroy() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// A scratch buffer of a handle that the kernels of one call write and read, and that kernels
// of the previous call, queued on any stream, may still be reading.  begin orders stream `s`
// after the previous call's end and returns at least `need` elements: the buffer grows only
// after the host has waited for that end too, since the free would pull the memory from
// under a queued reader.  end marks this call's last use.  Buffers of fixed size that the same
// calls rewrite (the AD tangent tables) are ordered by the same begin / end pair.
template <typename T>
class OrderedScratch {
public:
    T* begin(hipStream_t s, size_t need) {
        const bool had = done_.get() != nullptr;
        if (!had) done_.create();
        else hip_check(hipStreamWaitEvent(s, done_.get(), 0), "hipStreamWaitEvent");
        if (buf_.size() < need) {
            if (had) hip_check(hipEventSynchronize(done_.get()), "hipEventSynchronize");
            buf_.alloc(need);   // frees the old block first
        }
        return buf_.get();
    }
    void end(hipStream_t s) { hip_check(hipEventRecord(done_.get(), s), "hipEventRecord"); }

private:
    DeviceBuffer<T> buf_;
    DeviceEvent done_;
};

// ---------------------------------------------------------------- the launcher
// What a batch entry point launches with: the handle's device made current for the scope of
// the call, its device state and the caller's stream.  Handle: sunsky_emitter or
// sunsky_sequence (device, mod, d_state, precision, require_device(), xform_form(stream)).
template <typename Handle>
struct Launcher {
    const Handle* h;
    DeviceScope scope;
    const SunskyKArgs* K;
    hipStream_t s;
    Launcher(const Handle* handle, void* stream)
        : h(handle), scope(handle->device), K(handle->d_state.get()), s((hipStream_t)stream) {   // host-only: no device to scope
        h->require_device();
    }
    int form(KernelId k) const { return kKernels[k].forms == PLAIN ? 0 : h->xform_form(s); }

    // Kernel k over n samples on the table's grid.  dir: the eval_direction form (wo = d).
    void run(KernelId k, size_t n, void** args, bool dir = false) const {
        run_kernel(h->mod, form(k), h->precision, k, n, args, s, dir);
    }
    // Kernel k on a grid the call site fixes; precision < 0: the handle's
    void launch(KernelId k, unsigned grid, unsigned block, void** args, unsigned dyn_lds = 0, int precision = -1) const {
        capi::launch(h->mod->fn[form(k)][precision < 0 ? h->precision : precision][k], grid, block, s, args, dyn_lds);
    }
};

// ---------------------------------------------------------------- shared argument checks
// Each returns SUNSKY_OK or fails with the message its callers have always given.

// A switch of the environment, on at "1...": read at every call, tests flip them
inline bool env_switch(const char* name) {
    const char* v = std::getenv(name);
    return v && v[0] == '1';
}
inline bool unsorted_sampling() { return env_switch("SUNSKY_AMD_UNSORTED_SAMPLING"); }
inline bool general_xform() { return env_switch("SUNSKY_AMD_GENERAL_XFORM"); }

// Broadcast wavelengths (host array): a spectral handle needs 1..32, an RGB one takes none
inline int check_broadcast_lambda(bool spec, const float* lam_host, int m, const char* spec_msg, const char* rgb_msg) {
    if (spec && (!lam_host || m < 1 || m > kMaxBroadcastLambda)) return fail(SUNSKY_ERROR_INVALID_VALUE, spec_msg);
    if (!spec && lam_host && m) return fail(SUNSKY_ERROR_INVALID_VALUE, rgb_msg);
    return SUNSKY_OK;
}

// The arguments of the two bake_latlong calls, and the angles of the pixel grid as
// dr::linspace(start, end, count) steps them: (end - start) / (count - 1) in fp32
inline int check_bake(bool spec, int width, int height, float theta0, float theta1, float phi0, float phi1,
                      const float* lam_host, int m, const float* out, size_t ostride, LatLong* G) {
    if (width < 1 || height < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "image size must be >= 1 x 1");
    if ((int64_t)width * height >= (int64_t)1 << 31) return fail(SUNSKY_ERROR_INVALID_VALUE, "image larger than 2^31 pixels");
    if (int rc = check_broadcast_lambda(spec, lam_host, m, "1..32 wavelengths required for a spectral bake",
                                        "RGB bake takes no wavelengths")) return rc;
    if (!out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null output pointer");
    if (ostride < (size_t)width * (size_t)height) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < width * height");
    *G = {width, height, theta0, height > 1 ? (theta1 - theta0) / (float)(height - 1) : 0.f,
          phi0, width > 1 ? (phi1 - phi0) / (float)(width - 1) : 0.f, nullptr};
    return SUNSKY_OK;
}
inline int check_sequence_lambda(bool spec, const float* lam_host, int m) {
    return check_broadcast_lambda(spec, lam_host, m, "1..32 broadcast wavelengths required for a spectral sequence",
                                  "an RGB sequence takes no wavelengths");
}

// An optional vec3 of planes: all three or none
template <typename Vec3>
int check_optional_vec3(const Vec3& v, const char* name) {
    if ((v.x != nullptr) != (v.y != nullptr) || (v.x != nullptr) != (v.z != nullptr))
        return fail(SUNSKY_ERROR_INVALID_VALUE, std::string(name) + " must be all-NULL or all-set");
    return SUNSKY_OK;
}

// Per-ray wavelength planes of eval and its derivatives: 1..16 for a spectral emitter.  An
// empty batch has no planes to point to: only the count is checked then.
inline int check_ray_planes(bool spec, const float* lam, int nlam, size_t n) {
    if (spec && ((n && !lam) || nlam < 1 || nlam > kMaxLambdaPerRay))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "spectral eval needs 1..16 wavelength planes");
    return SUNSKY_OK;
}
// ... and the strides of their output and wavelength planes, which matter from the second plane on
inline int check_ray_strides(bool spec, int nlam, size_t lstride, size_t ostride, size_t n) {
    const size_t nout = spec ? (size_t)nlam : 3;
    if (n && nout > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    if (n && spec && nlam > 1 && lstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "wl_stride < n");
    return SUNSKY_OK;
}

// What sunsky_sequence_create snapshots from its parent (sunsky_capi_emitter.cpp)
struct EmitterSnapshot {
    const SunskyModel& model;
    const SunskyKArgs& kargs;
    DeviceModule* mod;
    int device, precision;
};
EmitterSnapshot emitter_snapshot(const ::sunsky_emitter* e);

}  // namespace capi
}  // namespace sunsky
