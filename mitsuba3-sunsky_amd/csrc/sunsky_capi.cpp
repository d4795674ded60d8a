// sunsky_capi.cpp -- the C ABI (include/sunsky_amd.h): host staging through
// SunskyModel, device tables, and kernel launches through hipModule.
#include "sunsky_amd.h"

#include <dlfcn.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <sys/stat.h>

#include "sunsky_dataset.h"
#include "sunsky_errors.h"
#include "sunsky_kernel_args.h"
#include "sunsky_model.h"
#include "sunsky_profiler.h"
#include "sunsky_props.h"
#include "sunsky_types.h"

using namespace sunsky;

// ---------------------------------------------------------------- errors
namespace sunsky {
double hosek_solar_radiance(const std::string& datasets, double turbidity, double wavelength, double elevation,
                            double gamma);
}

namespace sunsky {
namespace capi {
std::string& last_error() {
    thread_local std::string g_error;
    return g_error;
}
}  // namespace capi
}  // namespace sunsky

namespace {
using namespace sunsky::capi;

// ---------------------------------------------------------------- paths
std::string library_dir() {
    Dl_info info;
    if (dladdr((const void*)&library_dir, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        size_t s = p.rfind('/');
        return s == std::string::npos ? std::string(".") : p.substr(0, s);
    }
    return ".";
}

bool file_exists(const std::string& p) {
    struct stat st;
    return ::stat(p.c_str(), &st) == 0;
}

std::string default_pack_path() {
    if (const char* env = std::getenv("SUNSKY_AMD_DATASET")) return env;
    std::string d = library_dir();
    for (const char* rel : {"/sunsky_datasets.pack", "/../data/sunsky_datasets.pack", "/data/sunsky_datasets.pack"})
        if (file_exists(d + rel)) return d + rel;
    return d + "/../data/sunsky_datasets.pack";
}

std::string code_object_path() {
    if (const char* env = std::getenv("SUNSKY_AMD_CODE_OBJECT")) return env;
    return library_dir() + "/sunsky_kernels.hsaco";
}

// The same kernels compiled with to_world / to_local as the identity (SS_XFORM_IDENTITY),
// launched for emitters whose to_world is the identity: the same bits without the
// per-direction identity test.  SUNSKY_AMD_CODE_OBJECT_IDENT (a probe build) replaces it.
std::string ident_code_object_path() {
    if (const char* env = std::getenv("SUNSKY_AMD_CODE_OBJECT_IDENT")) return env;
    const std::string path = library_dir() + "/sunsky_kernels_ident.hsaco";
    // an A/B run that overrides only the general module would otherwise time the installed
    // identity module for every identity-to_world emitter without noticing
    if (std::getenv("SUNSKY_AMD_CODE_OBJECT"))
        std::fprintf(stderr, "sunsky_amd: SUNSKY_AMD_CODE_OBJECT is set but SUNSKY_AMD_CODE_OBJECT_IDENT is not: "
                             "emitters with an identity to_world use %s\n", path.c_str());
    return path;
}

// An SS_XFORM_IDENTITY build exports sunsky_xform_identity_marker.  Such an object as the
// general module would drop every rotated to_world without an error, and a general build
// as the identity module would only be slower: both are refused at load.
void check_xform_form(hipModule_t mod, const std::string& path, bool want_identity) {
    hipFunction_t f = nullptr;
    const bool is_identity = hipModuleGetFunction(&f, mod, "sunsky_xform_identity_marker") == hipSuccess;
    (void)hipGetLastError();
    if (is_identity != want_identity)
        throw HipError("code object " + path + (is_identity
            ? " is an identity-to_world build (SS_XFORM_IDENTITY); it cannot serve emitters with a rotated to_world "
              "(SUNSKY_AMD_CODE_OBJECT takes a general build, SUNSKY_AMD_CODE_OBJECT_IDENT an identity build)"
            : " is not an identity-to_world build (SUNSKY_AMD_CODE_OBJECT_IDENT takes an SS_XFORM_IDENTITY build)"));
}

// ---------------------------------------------------------------- kernels
// The sampling kernels are instantiated per variant (RGB / spectral) so each
// carries only its own tables and registers.
//
// The kernel table, one row per kernel: X(id, name, workgroups per CU, dir, per).
//  * name: the code objects export name_fast and name_ref.
//  * workgroups per CU: the cap of the grid-stride launches, sized to fill every CU several
//    times over (cdna_hip_programming.md Guideline 11).  From the tools/kbench.cpp sweep on
//    MI355X (profiles/r01_v2_kbench_grid_sweep.log): RGB eval 64 (60.4 us vs 64.9 us at 16
//    for 16M directions), spectral 64, sampling 64 (profiles/r01_v5_kbench.log,
//    r01_v7_tune.log); sample_ray 32, from the sweep over 8/16/32/64
//    (profiles/r03_v18_kbench_grid_ray_wavelengths.log); 16 where no sweep is recorded.  The
//    sequence kernels (one ray per lane, bound by VALU issue, not memory) take 64: one step per
//    lane up to 4M rays, where the cap only bounds the grid.  The sequence VJP kernels take 16:
//    every wave owns a row of the reduction workspace (sunsky_kernel_args.h), so fewer, longer
//    workgroups keep the workspace and the reduce pass small.
//  * dir: the eval kernels are instantiated twice: eval(si) negates wi at compile time,
//    eval_direction(ds) uses ds.d as is (name_dir_fast, name_dir_ref).
//  * per: samples per work item: 4 consecutive directions per lane in the VEC = 4 kernels
//    (their batches are multiples of 4); in the wave-sorted kernels one wave takes a window
//    of 4 (RGB) or 3 (spectral) x 64 samples.
#define SUNSKY_KERNELS(X)                                                                          \
    X(EVAL_RGB_V4, "sunsky_eval_rgb_v4", 64, true, 4)                                              \
    X(EVAL_RGB_V1, "sunsky_eval_rgb_v1", 64, true, 1)                                              \
    X(EVAL_SPEC_BCAST_V4, "sunsky_eval_spec_bcast_v4", 64, false, 4)                               \
    X(EVAL_SPEC_BCAST_V1, "sunsky_eval_spec_bcast_v1", 64, false, 1)                               \
    X(EVAL_SPEC_NODES_V4, "sunsky_eval_spec_nodes_v4", 64, false, 4)                               \
    X(EVAL_SPEC_RAYS_V4, "sunsky_eval_spec_rays_v4", 64, true, 4)                                  \
    X(EVAL_SPEC_RAYS_V1, "sunsky_eval_spec_rays_v1", 64, true, 1)                                  \
    X(EVAL_SPEC_RAYS4_V4, "sunsky_eval_spec_rays4_v4", 64, true, 4)                                \
    X(PDF_DIRECTION_V4, "sunsky_pdf_direction_v4", 64, false, 4)                                   \
    X(PDF_DIRECTION_V1, "sunsky_pdf_direction_v1", 64, false, 1)                                   \
    X(SAMPLE_DIRECTION_RGB, "sunsky_sample_direction_rgb", 64, false, 1)                           \
    X(SAMPLE_DIRECTION_RGB_LEAN, "sunsky_sample_direction_rgb_lean", 64, false, 4)                 \
    X(SAMPLE_DIRECTION_RGB_LEAN_PLAIN, "sunsky_sample_direction_rgb_lean_plain", 64, false, 1)     \
    X(SAMPLE_DIRECTION_RGB_FULL_SORTED, "sunsky_sample_direction_rgb_full_sorted", 64, false, 4)   \
    X(SAMPLE_DIRECTION_RGB_POS_SORTED, "sunsky_sample_direction_rgb_pos_sorted", 64, false, 4)     \
    X(SAMPLE_DIRECTION_SPEC, "sunsky_sample_direction_spec", 64, false, 1)                         \
    X(SAMPLE_DIRECTION_SPEC_LEAN, "sunsky_sample_direction_spec_lean", 64, false, 1)               \
    X(SAMPLE_DIRECTION_SPEC_LEAN4_SORTED, "sunsky_sample_direction_spec_lean4_sorted", 64, false, 3) \
    X(SAMPLE_DIRECTION_SPEC_POS_SORTED, "sunsky_sample_direction_spec_pos_sorted", 64, false, 3)   \
    X(SAMPLE_RAY_RGB, "sunsky_sample_ray_rgb", 32, false, 1)                                       \
    X(SAMPLE_RAY_RGB_SORTED, "sunsky_sample_ray_rgb_sorted", 64, false, 4)                         \
    X(SAMPLE_RAY_SPEC, "sunsky_sample_ray_spec", 32, false, 1)                                     \
    X(SAMPLE_WAVELENGTHS_RGB, "sunsky_sample_wavelengths_rgb", 16, false, 1)                       \
    X(SAMPLE_WAVELENGTHS_SPEC, "sunsky_sample_wavelengths_spec", 64, false, 1)                     \
    X(BAKE_RGB, "sunsky_bake_latlong_rgb", 64, false, 1)                                           \
    X(BAKE_SPEC, "sunsky_bake_latlong_spec", 64, false, 1)                                         \
    X(DIRECT_DIFFUSE_RGB, "sunsky_direct_diffuse_rgb", 64, false, 1)                               \
    X(DIRECT_DIFFUSE_SPEC, "sunsky_direct_diffuse_spec", 64, false, 1)                             \
    X(DIRECT_DIFFUSE_RAYS, "sunsky_direct_diffuse_rays", 64, false, 1)                             \
    X(DIRECT_CONDUCTOR_RGB, "sunsky_direct_conductor_rgb", 64, false, 1)                           \
    X(DIRECT_CONDUCTOR_SPEC, "sunsky_direct_conductor_spec", 64, false, 1)                         \
    X(DIRECT_CONDUCTOR_RAYS, "sunsky_direct_conductor_rays", 64, false, 1)                         \
    X(SEQUENCE_EVAL_RGB, "sunsky_sequence_eval_rgb", 64, false, 1)                                 \
    X(SEQUENCE_EVAL_SPEC, "sunsky_sequence_eval_spec", 64, false, 1)                               \
    X(SEQUENCE_BAKE_RGB, "sunsky_sequence_bake_rgb", 64, false, 1)                                 \
    X(SEQUENCE_BAKE_SPEC, "sunsky_sequence_bake_spec", 64, false, 1)                               \
    X(SEQUENCE_SAMPLE_RGB, "sunsky_sequence_sample_rgb", 64, false, 1)                             \
    X(SEQUENCE_SAMPLE_SPEC, "sunsky_sequence_sample_spec", 64, false, 1)                           \
    X(SEQUENCE_PDF, "sunsky_sequence_pdf", 64, false, 1)                                           \
    X(SEQUENCE_EVAL_VJP_RGB, "sunsky_sequence_eval_vjp_rgb", kSeqGradBlocksPerCu, false, 1)        \
    X(SEQUENCE_EVAL_VJP_SPEC, "sunsky_sequence_eval_vjp_spec", kSeqGradBlocksPerCu, false, 1)      \
    X(SEQUENCE_IRRADIANCE_RGB, "sunsky_sequence_irradiance_rgb", 64, false, 2)                     \
    X(SEQUENCE_IRRADIANCE_SPEC, "sunsky_sequence_irradiance_spec", 64, false, 2)                   \
    X(SEQUENCE_IRRADIANCE_HORIZON_RGB, "sunsky_sequence_irradiance_horizon_rgb", 64, false, 2)     \
    X(SEQUENCE_IRRADIANCE_HORIZON_SPEC, "sunsky_sequence_irradiance_horizon_spec", 64, false, 2)   \
    X(SEQUENCE_IRRADIANCE_VJP_NORMAL_RGB, "sunsky_sequence_irradiance_vjp_normal_rgb", 64, false, 2)   \
    X(SEQUENCE_IRRADIANCE_VJP_NORMAL_SPEC, "sunsky_sequence_irradiance_vjp_normal_spec", 64, false, 2) \
    X(SEQUENCE_IRRADIANCE_ADJOINT, "sunsky_sequence_irradiance_adjoint", kSeqIrrGradAdjointBlocksPerCu, false, 1) \
    X(SEQUENCE_IRRADIANCE_GRAD_FOLD, "sunsky_sequence_irradiance_grad_fold", kSeqIrrGradFoldBlocksPerCu, false, 1) \
    X(DEBUG_SUN_SEGMENTS, "sunsky_debug_sun_segments", 16, false, 1)

#define X(id, name, wg, dir, per) K_##id,
enum KernelId { SUNSKY_KERNELS(X) K_COUNT };
#undef X
struct KernelInfo {
    const char* name;
    int blocks_per_cu;
    bool dir_form;
    int per_item;
};
#define X(id, name, wg, dir, per) {name, wg, dir, per},
constexpr KernelInfo kKernels[] = {SUNSKY_KERNELS(X)};
#undef X
static_assert(sizeof(kKernels) / sizeof(kKernels[0]) == K_COUNT, "one table row per KernelId");

struct DeviceModule {
    hipModule_t module = nullptr, module_ident = nullptr;
    // [identity to_world][precision][kernel]: [1] from sunsky_kernels_ident.hsaco
    hipFunction_t fn[2][2][K_COUNT] = {};
    hipFunction_t fn_dir[2][2][K_COUNT] = {};   // eval_direction forms (wo = +d) of the eval kernels
    hipFunction_t jvp_rgb = nullptr, jvp_spec = nullptr;   // eval_jvp (reference operation order)
    hipFunction_t vjp_rgb = nullptr, vjp_spec = nullptr, grad_reduce = nullptr;   // eval_vjp
    hipFunction_t jvp_dir_rgb = nullptr, jvp_dir_spec = nullptr;   // eval_jvp_dir / eval_vjp_dir (d eval / d wi)
    hipFunction_t vjp_dir_rgb = nullptr, vjp_dir_spec = nullptr;
    hipFunction_t latlong_tables = nullptr;                                     // bake_latlong
    hipFunction_t stage_radiance = nullptr, quad_points = nullptr, quad_finish = nullptr;   // parameters_changed
    hipFunction_t stage_tangent = nullptr;                                      // eval_jvp / eval_vjp tables
    hipFunction_t stage_sequence = nullptr;                                     // sequence_create
    hipFunction_t sequence_table = nullptr, sequence_suns = nullptr;            // sequence_prepare_sampling
    hipFunction_t stage_sequence_grad = nullptr, sequence_grad_reduce = nullptr;   // sequence_prepare_grad / _eval_vjp
    hipFunction_t irradiance_table = nullptr, irradiance_flux = nullptr;        // sequence_prepare_irradiance
    int cu_count = 256;
};

std::mutex g_module_mutex;
std::map<int, DeviceModule*> g_modules;

DeviceModule* module_for_device(int dev) {
    std::lock_guard<std::mutex> lock(g_module_mutex);
    auto it = g_modules.find(dev);
    if (it != g_modules.end()) return it->second;
    std::unique_ptr<DeviceModule> m(new DeviceModule());
    const std::string path = code_object_path(), ipath = ident_code_object_path();
    for (const std::string& p : {path, ipath})
        if (!file_exists(p)) throw HipError("kernel code object not found: " + p + " (run the build)");
    hip_check(hipModuleLoad(&m->module, path.c_str()), "hipModuleLoad(sunsky_kernels.hsaco)");
    check_xform_form(m->module, path, false);
    hip_check(hipModuleLoad(&m->module_ident, ipath.c_str()), "hipModuleLoad(sunsky_kernels_ident.hsaco)");
    check_xform_form(m->module_ident, ipath, true);
    auto get = [](hipFunction_t* f, hipModule_t mod, const std::string& name) {
        hip_check(hipModuleGetFunction(f, mod, name.c_str()), name.c_str());
    };
    for (int id = 0; id < 2; ++id)
        for (int p = 0; p < 2; ++p)
            for (int k = 0; k < K_COUNT; ++k) {
                hipModule_t mod = id ? m->module_ident : m->module;
                const std::string name = kKernels[k].name, prec = p == SUNSKY_PRECISION_FAST ? "_fast" : "_ref";
                get(&m->fn[id][p][k], mod, name + prec);
                if (kKernels[k].dir_form) get(&m->fn_dir[id][p][k], mod, name + "_dir" + prec);
            }
    get(&m->jvp_rgb, m->module, "sunsky_eval_jvp_rgb");
    get(&m->jvp_spec, m->module, "sunsky_eval_jvp_spec");
    get(&m->vjp_rgb, m->module, "sunsky_eval_vjp_rgb");
    get(&m->vjp_spec, m->module, "sunsky_eval_vjp_spec");
    get(&m->grad_reduce, m->module, "sunsky_grad_reduce");
    get(&m->jvp_dir_rgb, m->module, "sunsky_eval_jvp_dir_rgb");
    get(&m->jvp_dir_spec, m->module, "sunsky_eval_jvp_dir_spec");
    get(&m->vjp_dir_rgb, m->module, "sunsky_eval_vjp_dir_rgb");
    get(&m->vjp_dir_spec, m->module, "sunsky_eval_vjp_dir_spec");
    get(&m->latlong_tables, m->module, "sunsky_latlong_tables");
    get(&m->stage_tangent, m->module, "sunsky_stage_tangent");
    get(&m->stage_sequence, m->module, "sunsky_stage_sequence");
    get(&m->sequence_table, m->module, "sunsky_sequence_table");
    get(&m->sequence_suns, m->module, "sunsky_sequence_suns");
    get(&m->stage_sequence_grad, m->module, "sunsky_stage_sequence_grad");
    get(&m->sequence_grad_reduce, m->module, "sunsky_sequence_grad_reduce");
    get(&m->irradiance_table, m->module, "sunsky_sequence_irradiance_table");
    get(&m->irradiance_flux, m->module, "sunsky_sequence_irradiance_flux");
    get(&m->stage_radiance, m->module, "sunsky_stage_radiance");
    get(&m->quad_points, m->module, "sunsky_stage_quad_points");
    get(&m->quad_finish, m->module, "sunsky_stage_quad_finish");
    hip_check(hipDeviceGetAttribute(&m->cu_count, hipDeviceAttributeMultiprocessorCount, dev),
              "hipDeviceGetAttribute");
    DeviceModule* raw = m.release();
    g_modules[dev] = raw;
    return raw;
}

constexpr int kBlock = 256;

// Grid of a grid-stride launch of kernel k over `work_items`: one thread each, up to the
// table's workgroups per CU.  SUNSKY_AMD_BLOCKS_PER_CU overrides every kernel's (read once).
unsigned grid_for(const DeviceModule* m, KernelId k, size_t work_items) {
    static const int env = [] {
        const char* e = std::getenv("SUNSKY_AMD_BLOCKS_PER_CU");
        return e ? std::max(1, std::atoi(e)) : 0;
    }();
    size_t need = (work_items + kBlock - 1) / kBlock;
    size_t cap = (size_t)m->cu_count * (size_t)(env ? env : kKernels[k].blocks_per_cu);
    return (unsigned)std::max<size_t>(1, std::min(need, cap));
}

void launch(hipFunction_t f, unsigned grid, hipStream_t stream, void** args, unsigned dyn_lds = 0) {
    hip_check(hipModuleLaunchKernel(f, grid, 1, 1, kBlock, 1, 1, dyn_lds, stream, args, nullptr),
              "hipModuleLaunchKernel");
}

// The 11-node spectral kernel with more than one step per lane (configs[4]'s 64M directions
// per GPU): unused dynamic LDS that holds it to 5 workgroups (5 waves/SIMD) per CU.  Fewer
// concurrent 11-plane write streams per CU write HBM faster there: 64M x 11 cold, 774 ->
// 750 us at 5 and 745 us at 4 workgroups per CU, 806 us at 2; at one step per lane (16M)
// neutral (profiles/r06_v8_nodes_occupancy_cold.log, r06_v7_ab_nodes_lds_cap.log).
constexpr unsigned kNodesLdsCap = 32000;

// Kernel k of code object `form` (1: identity to_world) and `precision` over n samples on
// stream s.  dir: the eval_direction form (wo = d) of an eval kernel.
void run_kernel(const DeviceModule* mod, int form, int precision, KernelId k, size_t n, void** args, hipStream_t s,
                bool dir = false) {
    const size_t per = (size_t)kKernels[k].per_item, items = (n + per - 1) / per;
    const unsigned grid = grid_for(mod, k, items);
    const bool multi_step = items > (size_t)grid * kBlock;
    const auto& fns = dir ? mod->fn_dir : mod->fn;
    launch(fns[form][precision][k], grid, s, args, k == K_EVAL_SPEC_NODES_V4 && multi_step ? kNodesLdsCap : 0u);
}

// The VEC = 4 kernels move 16 bytes per lane and plane (4 mask bytes).  How many of a batch's
// n samples they can take: the multiple of 4 below n when every plane of `planes` is 16-byte
// aligned, every plane stride of `strides` a multiple of 4 and the mask 4-byte aligned, else 0.
size_t vec4_count(size_t n, std::initializer_list<const void*> planes, std::initializer_list<size_t> strides,
                  const uint8_t* active) {
    bool vec = n >= 4 && (!active || ((uintptr_t)active & 3u) == 0);
    for (const void* p : planes) vec = vec && ((uintptr_t)p & 15u) == 0;
    for (size_t s : strides) vec = vec && (s % 4) == 0;
    return vec ? (n & ~(size_t)3) : 0;
}

// part(offset, count, vec): the VEC = 4 body over [0, n4), then the VEC = 1 tail over [n4, n)
template <typename F>
void vec4_then_tail(size_t n, size_t n4, F&& part) {
    if (n4) part((size_t)0, n4, true);
    if (n4 < n) part(n4, n - n4, false);
}

// normalized_wavelengths / floor2int / lerp factor of eval, sunsky.cpp:326-332
LambdaSet make_lambda_set(const float* lam, int m) {
    LambdaSet L;
    std::memset(&L, 0, sizeof(L));
    L.m = m;
    for (int k = 0; k < m; ++k) {
        float nw = (lam[k] - kWavelength0) / kWavelengthStep;
        bool valid = (0.f <= nw) && (nw <= (float)(kNbWavelengths - 1));
        int lo = valid ? (int)std::floor(nw) : 0;
        L.lo[k] = lo;
        L.f[k] = valid ? nw - (float)lo : -1.f;
    }
    return L;
}

// Makes the emitter's device current for the scope of an entry point: every
// allocation, event and launch of an emitter happens on its own GPU whatever the
// caller's current device is.
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

}  // namespace

// ---------------------------------------------------------------- handles
struct sunsky_props {
    Properties props;
};

struct sunsky_emitter {
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
    SunskyKArgs* d_state = nullptr;
    float* d_sun_table = nullptr;
    float* d_sun_ld = nullptr;
    float* d_datasets = nullptr;          // sky params | sky radiance | sun table | quadrature x | w
    const float *d_sky_params_ds = nullptr, *d_sky_rad_ds = nullptr, *d_sun_rad_ds = nullptr;
    const float *d_qx = nullptr, *d_qw = nullptr;
    float* d_quad_part = nullptr;         // quadrature row sums [2][200][nch]
    int* d_status = nullptr;              // device staging status (0 ok)
    static constexpr int kRing = 4;       // pinned host images of the state for the async copy
    SunskyKArgs* h_ring = nullptr;
    hipEvent_t ring_ev[kRing] = {};
    bool ring_used[kRing] = {};
    int ring_i = 0;
    bool restoring = false;                    // restaging the accepted state after a rejection
    int inject_faults = 0;                     // testing: stagings left that report a rejection
    mutable hipEvent_t stage_done = nullptr;   // recorded after the last device staging
    mutable float* d_jvp = nullptr;   // eval_jvp tangent tables (layout: sunsky_kernels.hip)
    mutable float* d_vjp = nullptr;   // eval_vjp basis-tangent tables
    mutable float* d_partials = nullptr;   // eval_vjp per-workgroup gradient partials
    mutable size_t partials_cap = 0;
    mutable float* d_bake = nullptr;       // bake_latlong angle tables
    mutable size_t bake_cap = 0;
    // AD tangent tables depend only on the emitter state: restaged when `rev` (bumped by
    // every staging) or, for the JVP, the requested tangent changes.  `ad_done` is recorded
    // after each AD launch; the next AD call's stream waits on it, so a later call on
    // another stream cannot overwrite d_jvp / d_partials under an in-flight kernel.  The
    // bakes order their angle tables the same way (`bake_done`).
    uint64_t rev = 0;
    mutable uint64_t vjp_rev = ~0ull, jvp_rev = ~0ull;
    mutable std::vector<float> jvp_key;
    mutable hipEvent_t ad_done = nullptr, bake_done = nullptr;

    static constexpr int kJvpFloats = kJvpSunOffset + kSunRgbTableSize;   // AD tangent buffers
    static constexpr int kVjpFloats = kVjpSunOffset + kSunRgbTableSize;

    // Allocations of a GPU emitter (once, at creation): state, tables, the raw datasets
    // the staging kernels read, quadrature nodes, scratch, pinned ring, events.
    void init_device() {
        const bool spec = model->variant() == kSpectral;
        hip_check(hipMalloc(&d_state, sizeof(SunskyKArgs)), "hipMalloc");
        hip_check(hipMalloc(&d_sun_table, sizeof(float) * kSunRgbTableSize), "hipMalloc");
        hip_check(hipMalloc(&d_sun_ld, sizeof(float) * kNbWavelengths * kNbSunLdParams), "hipMalloc");
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
        hip_check(hipMalloc(&d_datasets, sizeof(float) * all.size()), "hipMalloc");
        hip_check(hipMemcpy(d_datasets, all.data(), sizeof(float) * all.size(), hipMemcpyHostToDevice), "hipMemcpy");
        d_sky_params_ds = d_datasets;
        d_sky_rad_ds = d_sky_params_ds + sp.size();
        d_sun_rad_ds = d_sky_rad_ds + sr.size();
        d_qx = d_sun_rad_ds + su.size();
        d_qw = d_qx + qx.size();
        const std::vector<float>& ld = model->sun_ld();
        if (spec)
            hip_check(hipMemcpy(d_sun_ld, ld.data(), sizeof(float) * std::min<size_t>(ld.size(), kNbWavelengths * kNbSunLdParams),
                                hipMemcpyHostToDevice), "hipMemcpy");
        const size_t nq = qx.size();
        hip_check(hipMalloc(&d_quad_part, sizeof(float) * 2 * nq * model->nch()), "hipMalloc");
        hip_check(hipMalloc(&d_status, sizeof(int)), "hipMalloc");
        hip_check(hipMemset(d_status, 0, sizeof(int)), "hipMemset");
        hip_check(hipHostMalloc((void**)&h_ring, sizeof(SunskyKArgs) * kRing, hipHostMallocDefault), "hipHostMalloc");
        for (int i = 0; i < kRing; ++i)
            hip_check(hipEventCreateWithFlags(&ring_ev[i], hipEventDisableTiming), "hipEventCreate");
        hip_check(hipEventCreateWithFlags(&stage_done, hipEventDisableTiming), "hipEventCreate");
    }

    // parameters_changed on the device, ordered on `s`: the host-staged part of the
    // state (geometry, TGMM, discrete distribution) by an async copy from a pinned image,
    // then the staging kernels write the sky channels, the sun table and (JIT) the
    // sampling weight and wavelength distribution.  Nothing here waits for the device,
    // except for a pinned image still in flight kRing updates later.
    void stage_async(hipStream_t s) {
        kargs = model->kargs();
        kargs.sun_table = d_sun_table;
        kargs.sun_ld = d_sun_ld;
        const int slot = ring_i;
        ring_i = (ring_i + 1) % kRing;
        if (ring_used[slot]) hip_check(hipEventSynchronize(ring_ev[slot]), "hipEventSynchronize");
        h_ring[slot] = kargs;
        hip_check(hipMemcpyAsync(d_state, &h_ring[slot], sizeof(SunskyKArgs), hipMemcpyHostToDevice, s),
                  "hipMemcpyAsync");
        hip_check(hipEventRecord(ring_ev[slot], s), "hipEventRecord");
        ring_used[slot] = true;
        const bool spec = model->variant() == kSpectral;
        StageArgs A;
        std::memset(&A, 0, sizeof(A));
        A.state = d_state;
        A.sun_table = d_sun_table;
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
        hip_check(hipModuleLaunchKernel(mod->stage_radiance, 1, 1, 1, 256, 1, 1, 0, s, sargs, nullptr),
                  "hipModuleLaunchKernel(sunsky_stage_radiance)");
        if (model->semantics() == kJit) {
            QuadArgs Q;
            std::memset(&Q, 0, sizeof(Q));
            Q.state = d_state;
            Q.qx = d_qx;
            Q.qw = d_qw;
            Q.rows = d_quad_part;
            Q.nq = 200;
            Q.nch = model->nch();
            std::memcpy(Q.cie_y, model->cie_y(), sizeof(Q.cie_y));
            Q.sky_scale = model->sky_scale();
            Q.sun_scale = model->sun_scale();
            Q.status = d_status;
            void* qargs[] = {&Q};
            static_assert(200 <= kQuadBlock, "one quadrature row per workgroup");
            hip_check(hipModuleLaunchKernel(mod->quad_points, (unsigned)Q.nq, 1, 1, kQuadBlock, 1, 1, 0, s, qargs, nullptr),
                      "hipModuleLaunchKernel(sunsky_stage_quad_points)");
            hip_check(hipModuleLaunchKernel(mod->quad_finish, 1, 1, 1, 256, 1, 1, 0, s, qargs, nullptr),
                      "hipModuleLaunchKernel(sunsky_stage_quad_finish)");
        }
        if (inject_faults > 0 && model->semantics() == kJit && !restoring) {   // sunsky_emitter_inject_staging_fault
            --inject_faults;
            hip_check(hipMemsetAsync(d_status, 1, 1, s), "hipMemsetAsync");
        }
        hip_check(hipEventRecord(stage_done, s), "hipEventRecord");
        ++rev;
    }

    // Bring the device-staged fields back into the host model (get_info / get_table /
    // to_string): waits for the last staging only.
    void sync_host() const {
        if (!model->radiance_stale() || !d_state) return;
        DeviceScope g(device);
        hip_check(hipEventSynchronize(stage_done), "hipEventSynchronize");
        SunskyKArgs dk;
        hip_check(hipMemcpy(&dk, d_state, sizeof(dk), hipMemcpyDeviceToHost), "hipMemcpy");
        std::vector<float> st(kSunRgbTableSize);
        hip_check(hipMemcpy(st.data(), d_sun_table, sizeof(float) * st.size(), hipMemcpyDeviceToHost), "hipMemcpy");
        int status = 0;
        hip_check(hipMemcpy(&status, d_status, sizeof(int), hipMemcpyDeviceToHost), "hipMemcpy");
        auto* self = const_cast<sunsky_emitter*>(this);
        if (status) {
            // A device staging since the last read-back rejected its update (a negative
            // wavelength-distribution node, the check of ContinuousDistribution's
            // constructor); the status is sticky, so which one is unknown.  As the reference
            // throws from parameters_changed and keeps its old state: restore the parameters
            // of the last staging known to be accepted, restage them, report the error once.
            hip_check(hipMemset(d_status, 0, sizeof(int)), "hipMemset");
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
        const char* g = std::getenv("SUNSKY_AMD_GENERAL_XFORM");
        if (!kargs.identity_xform || (g && g[0] == '1')) return 0;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        hip_check(hipStreamIsCapturing(s, &cs), "hipStreamIsCapturing");
        return cs == hipStreamCaptureStatusNone ? 1 : 0;
    }
    // Batch calls need the emitter's device state: a host-only emitter
    // (sunsky_emitter_create_host) has none and rejects them.
    void require_device() const {
        if (!mod) throw std::invalid_argument("host-only emitter (sunsky_emitter_create_host) cannot launch kernels");
    }

    ~sunsky_emitter() {
        if (device < 0) return;
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != device) (void)hipSetDevice(device);
        // a destroyed emitter may still be read by launches in flight on any stream
        (void)hipDeviceSynchronize();
        for (void* p : {(void*)d_state, (void*)d_sun_table, (void*)d_sun_ld, (void*)d_datasets, (void*)d_quad_part,
                        (void*)d_status, (void*)d_jvp, (void*)d_vjp, (void*)d_partials, (void*)d_bake})
            if (p) (void)hipFree(p);
        if (h_ring) (void)hipHostFree(h_ring);
        for (hipEvent_t ev : ring_ev)
            if (ev) (void)hipEventDestroy(ev);
        for (hipEvent_t ev : {stage_done, ad_done, bake_done})
            if (ev) (void)hipEventDestroy(ev);
        if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
    }

    // Order this AD call after the previous one (any stream), then mark its end.
    void ad_begin(hipStream_t st) const {
        if (!ad_done) hip_check(hipEventCreateWithFlags(&ad_done, hipEventDisableTiming), "hipEventCreate");
        else hip_check(hipStreamWaitEvent(st, ad_done, 0), "hipStreamWaitEvent");
    }
    void ad_end(hipStream_t st) const { hip_check(hipEventRecord(ad_done, st), "hipEventRecord"); }
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
        const unsigned grid = (unsigned)((A.total + 255) / 256);
        hip_check(hipModuleLaunchKernel(mod->stage_tangent, grid, 1, 1, 256, 1, 1, 0, st, args, nullptr),
                  "hipModuleLaunchKernel(sunsky_stage_tangent)");
    }
};

// What a batch entry point launches with: the emitter's device made current for the scope
// of the call, its device state and the caller's stream.
struct Launcher {
    const sunsky_emitter* e;
    DeviceScope scope;
    const SunskyKArgs* K;
    hipStream_t s;
    Launcher(const sunsky_emitter* em, void* stream)
        : e(em), scope(em->device), K(em->d_state), s((hipStream_t)stream) {   // a host-only emitter: no device to scope
        e->require_device();
    }

    // Kernel k over n samples.  dir: the eval_direction form (wo = d) of an eval kernel.
    void run(KernelId k, size_t n, void** args, bool dir = false) const {
        run_kernel(e->mod, e->xform_form(s), e->precision, k, n, args, s, dir);
    }
};

// ---------------------------------------------------------------- sequences
// K frames over a snapshot of one emitter (sunsky_amd.h, "frame sequences").  The object
// owns everything its kernels read: a copy of the emitter's state block (geometry, scales,
// aperture, segment thresholds), the frame records, the raw sun dataset the disc lanes lerp
// from, and the limb-darkening table.  Nothing points back to the emitter.
struct sunsky_sequence {
    SunskyKArgs kargs;                       // the snapshot (host); sun_ld -> d_sun_ld on the device
    int count = 0, nch = 0, variant = 0;
    int precision = SUNSKY_PRECISION_FAST;
    int device = -1;                         // -1: host-only (no batch calls)
    DeviceModule* mod = nullptr;
    std::vector<unsigned char> records;      // SeqFrame<nch>[count], staged (host mirror: get_frame)
    size_t rec_bytes = 0;
    int sun_block = 0;
    SunskyKArgs* d_state = nullptr;
    void* d_frames = nullptr;
    float* d_sun_rad = nullptr;
    float* d_sun_ld = nullptr;
    mutable float* d_bake = nullptr;         // bake_latlong angle tables, ordered as the emitter's
    mutable size_t bake_cap = 0;
    mutable hipEvent_t bake_done = nullptr;
    // sampling (prepare_sampling): the snapshot's luminance weights and, for host-only
    // sequences, the tables the disc term reads; then the distribution itself
    float cie_y[kNbWavelengths] = {0};
    std::vector<float> h_sun_rad, h_sun_ld;
    int samp_nz = 0, samp_nphi = 0;          // 0: not prepared
    float samp_w_sky = 0.f, samp_sky_mass = 0.f, samp_sun_mass = 0.f;
    std::vector<float> samp_f, samp_row_cdf, samp_cell_cdf, samp_q, samp_frame_cdf, samp_B;
    float* d_samp = nullptr;                 // f, row_cdf, cell_cdf, frame_cdf, suns in one block
    SeqSampling samp = {};
    // what update / prepare_grad restage from: the frames as given (defaults resolved) and the
    // parent's albedo, to_local and raw sky datasets (host copies for host-only sequences, the
    // sequence's own device copy otherwise: the parent may be gone)
    std::vector<float> in_dirs, in_turbidity, in_weights;
    std::vector<float> albedo;
    double to_local_d[9] = {0};
    std::vector<float> h_sky_params_ds, h_sky_rad_ds;
    float* d_sky_ds = nullptr;               // sky params | sky radiance
    const float *d_sky_params_ds = nullptr, *d_sky_rad_ds = nullptr;
    // gradients (prepare_grad): the records' host mirror (frame_tangent), the device records,
    // the staging scalars and the reduction workspace of the largest grid eval_vjp launches
    bool grad_ready = false;
    std::vector<unsigned char> grads;        // SeqGradFrame<nch>[count]
    void* d_grads = nullptr;
    TangentStage* d_grad_stages = nullptr;
    float* d_grad_rows = nullptr;
    unsigned grad_max_grid = 0;
    // irradiance (prepare_irradiance): the tables as read back (R_p and F_k[p], unweighted) and
    // the staged device image the hot path walks (cell records, then sun records)
    int irr_nz = 0, irr_nphi = 0, irr_planes = 0;   // 0: not prepared
    float irr_omega = 0.f;
    std::vector<float> irr_sky, irr_flux;
    float* d_irr = nullptr;
    SeqIrradiance irr = {};
    // the grid column j_k of every frame's sun (irradiance_horizon's sectors); on the device the
    // columns of the image's suns, in the image's order, behind the image
    std::vector<int> irr_sun_cols;
    const int* d_irr_sun_cols = nullptr;
    LambdaSet irr_L = {};                    // the spectral planes' wavelengths (the weight gradient's sky terms)
    // gradients of the irradiance (prepare_irradiance_grad): asked for once (sticky: a later
    // prepare_irradiance restages it), staged for the current tables when irr_grad_ready
    bool irr_grad_wanted = false, irr_grad_ready = false;
    float* d_irr_grad = nullptr;             // every frame's sun | F_k[p] | the reduction workspace
    SeqIrrGrad irr_grad = {};
    size_t irr_grad_cap = 0;                 // the workspace bound in floats, as read at prepare time

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
    // The snapshot never changes, so an identity to_world takes the identity code object under
    // capture too (SUNSKY_AMD_GENERAL_XFORM=1: the general one always)
    int xform_form() const {
        const char* g = std::getenv("SUNSKY_AMD_GENERAL_XFORM");
        return kargs.identity_xform && !(g && g[0] == '1') ? 1 : 0;
    }
    SeqArgs args() const { return SeqArgs{d_frames, d_sun_rad, count, sun_block}; }

    ~sunsky_sequence() {
        if (device < 0) return;
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != device) (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();   // launches in flight may still read the records
        for (void* p : {(void*)d_state, d_frames, (void*)d_sun_rad, (void*)d_sun_ld, (void*)d_bake, (void*)d_samp,
                        (void*)d_sky_ds, d_grads, (void*)d_grad_stages, (void*)d_grad_rows, (void*)d_irr,
                        (void*)d_irr_grad})
            if (p) (void)hipFree(p);
        if (bake_done) (void)hipEventDestroy(bake_done);
        if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
    }
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
    hip_check(hipMemcpy(q->d_frames, q->records.data(), q->records.size(), hipMemcpyHostToDevice), "hipMemcpy");
    SeqStageArgs A;
    std::memset(&A, 0, sizeof(A));
    A.frames = q->d_frames;
    A.sky_params_ds = q->d_sky_params_ds;
    A.sky_rad_ds = q->d_sky_rad_ds;
    for (int c = 0; c < q->nch; ++c) A.albedo[c] = q->albedo[c];
    A.nch = q->nch;
    A.variant = q->variant;
    A.count = q->count;
    A.sky_scale = q->kargs.sky_scale;
    void* sargs[] = {&A};
    hip_check(hipModuleLaunchKernel(q->mod->stage_sequence, (unsigned)std::min(q->count, 65535), 1, 1, 256, 1, 1, 0, nullptr,
                                    sargs, nullptr), "hipModuleLaunchKernel(sunsky_stage_sequence)");
    hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    hip_check(hipMemcpy(q->records.data(), q->d_frames, q->records.size(), hipMemcpyDeviceToHost), "hipMemcpy");
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
    hip_check(hipMemcpy(q->d_grads, q->grads.data(), q->grads.size(), hipMemcpyHostToDevice), "hipMemcpy");
    hip_check(hipMemcpy(q->d_grad_stages, stages.data(), sizeof(TangentStage) * stages.size(), hipMemcpyHostToDevice),
              "hipMemcpy");
    SeqGradStageArgs A = {q->d_grads, q->d_grad_stages, q->d_sky_params_ds, q->d_sky_rad_ds, nch, q->count};
    void* args[] = {&A};
    hip_check(hipModuleLaunchKernel(q->mod->stage_sequence_grad, (unsigned)std::min(q->count, 65535), 1, 1, 256, 1, 1, 0,
                                    nullptr, args, nullptr), "hipModuleLaunchKernel(sunsky_stage_sequence_grad)");
    hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    hip_check(hipMemcpy(q->grads.data(), q->d_grads, q->grads.size(), hipMemcpyDeviceToHost), "hipMemcpy");
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
void seq_irradiance_host(const sunsky_sequence* q, int nz, int nphi, const LambdaSet& L, int planes, float s2,
                         std::vector<float>& sky_out, std::vector<float>& flux) {
    const SunskyKArgs& K = q->kargs;
    const bool rgb = q->variant == kRGB;
    const float cie = (float)kCieYNormalization;
    const size_t cells = (size_t)nz * (size_t)nphi;
    for (int i = 0; i < nz; ++i)
        for (int j = 0; j < nphi; ++j) {
            const float3_ wo = seq_cell_centre(nz, nphi, i, j);
            float acc[kSeqIrrMaxPlanes] = {0};
            for (int k = 0; k < q->count; ++k) {
                const SeqFrame<1>* h = seq_header(q, k);
                const SkyChannel* sky = seq_sky(q, k);
                const float gamma = unit_angle(mk3(h->sun_n[0], h->sun_n[1], h->sun_n[2]), wo);
                if (rgb) {
                    for (int c = 0; c < 3; ++c)
                        acc[c] = fmaf(h->weight, K.sky_scale * render_sky(sky[c], wo.z, gamma) * cie, acc[c]);
                    continue;
                }
                for (int p = 0; p < planes; ++p) {
                    const int lo = L.lo[p], hi = lo + 1 < kNbWavelengths ? lo + 1 : lo;
                    const float f = L.f[p];
                    if (!(f >= 0.f)) continue;
                    float v = K.sky_scale * render_sky(sky[lo], wo.z, gamma);
                    if (f != 0.f) v = lerpf_(v, K.sky_scale * render_sky(sky[hi], wo.z, gamma), f);
                    acc[p] = fmaf(h->weight, v, acc[p]);
                }
            }
            for (int p = 0; p < planes; ++p) sky_out[(size_t)p * cells + (size_t)i * nphi + j] = acc[p];
        }
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
// are now: every frame's local sun direction, the unweighted fluxes, and the workspace of the
// most slices the bound allows.  A host-only sequence only changes state.
void seq_stage_irradiance_grad(sunsky_sequence* q) {
    q->irr_grad_ready = false;
    if (q->device >= 0) {
        if (q->d_irr_grad) hip_check(hipFree(q->d_irr_grad), "hipFree");
        q->d_irr_grad = nullptr;
        const int planes = q->irr_planes, count = q->count;
        const size_t cells = (size_t)q->irr_nz * (size_t)q->irr_nphi, entries = cells + (size_t)count;
        q->irr_grad_cap = seq_irr_grad_cap();
        const size_t slices = seq_irr_grad_max_slices(planes, cells, count, q->irr_grad_cap);
        const size_t head = 4 * (size_t)count + (size_t)planes * count;
        std::vector<float> h(head, 0.f);
        for (int k = 0; k < count; ++k) {
            const SeqFrame<1>* f = seq_header(q, k);
            for (int a = 0; a < 3; ++a) h[4 * (size_t)k + a] = f->sun_n[a];
        }
        std::copy(q->irr_flux.begin(), q->irr_flux.end(), h.begin() + 4 * (size_t)count);
        hip_check(hipMalloc(&q->d_irr_grad, sizeof(float) * (head + slices * planes * entries)), "hipMalloc");
        hip_check(hipMemcpy(q->d_irr_grad, h.data(), sizeof(float) * head, hipMemcpyHostToDevice), "hipMemcpy");
        SeqIrrGrad& g = q->irr_grad;
        std::memset(&g, 0, sizeof(g));
        g.suns = q->d_irr_grad;
        g.flux = q->d_irr_grad + 4 * (size_t)count;
        g.rows = q->d_irr_grad + head;
        g.omega = q->irr_omega;
        g.count = count;
    }
    q->irr_grad_ready = true;
}

}  // namespace

extern "C" {

int sunsky_abi_version(void) { return SUNSKY_AMD_ABI_VERSION; }
const char* sunsky_last_error(void) { return last_error().c_str(); }

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
            hip_check(hipEventSynchronize(e->stage_done), "hipEventSynchronize");
            hip_check(hipMemcpy((char*)e->d_state + offsetof(SunskyKArgs, bs_center), bs, sizeof(bs),
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
    if (spec && (!lam || nlam < 1 || nlam > kMaxLambdaPerRay))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "spectral eval needs 1..16 wavelength planes");
    const size_t nout = spec ? (size_t)nlam : 3;
    if (nout > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    if (spec && nlam > 1 && lstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "wl_stride < n");
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
            // the wavelength planes too; their stride matters only when there is a second plane
            const size_t n4 = vec4_count(n, {w.x, w.y, w.z, out, lam}, {ostride, nlam == 1 ? 0 : lstride}, active);
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
        const size_t n4 = vec4_count(n, {w.x, w.y, w.z, out}, {ostride}, active);
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
    if ((it_p.x != nullptr) != (it_p.y != nullptr) || (it_p.x != nullptr) != (it_p.z != nullptr))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "it_p must be all-NULL or all-set");
    if ((ds_p.x != nullptr) != (ds_p.y != nullptr) || (ds_p.x != nullptr) != (ds_p.z != nullptr))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "ds_p must be all-NULL or all-set");
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
        const char* uns = std::getenv("SUNSKY_AMD_UNSORTED_SAMPLING");
        const bool unsorted = uns && uns[0] == '1';
        // SUNSKY_AMD_SORTED_GENERAL_SAMPLING=1: the masked general RGB call through the wave-sorted
        // kernel (10 % slower than the unsorted one; bitwise tests only)
        const char* sgs = std::getenv("SUNSKY_AMD_SORTED_GENERAL_SAMPLING");
        const bool sorted_general = sgs && sgs[0] == '1' && !unsorted;
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
        const char* uns = std::getenv("SUNSKY_AMD_UNSORTED_SAMPLING");
        const bool unsorted = uns && uns[0] == '1';
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
    // an empty batch has no planes to point to (as sunsky_eval): only the count is checked then
    if (spec && ((n && !lam) || nlam < 1 || nlam > kMaxLambdaPerRay))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "spectral eval needs 1..16 wavelength planes");
    const size_t nout = spec ? (size_t)nlam : 3;
    if (n && (!wi.x || !wi.y || !wi.z || !out || !d_out))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / output pointer");
    if (n && nout > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    if (n && spec && nlam > 1 && lstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "wl_stride < n");
    return guarded([&] {
        std::vector<float> key(tangent, tangent + std::max(0, tangent_count));
        key.push_back((float)param);
        const bool stage = !e->d_jvp || e->jvp_rev != e->rev || key != e->jvp_key;
        TangentStage ts;
        if (stage || n == 0) ts = e->model->tangent_stage(param, tangent, tangent_count);   // validates param / count
        if (n == 0) return;
        Launcher lc(e, stream);
        hipStream_t st = lc.s;
        e->ad_begin(st);   // ordered after the previous AD call (which may read d_jvp), any stream
        if (stage) {   // the tangent tables, staged on the device (sunsky_stage_tangent)
            if (!e->d_jvp) hip_check(hipMalloc(&e->d_jvp, sizeof(float) * sunsky_emitter::kJvpFloats), "hipMalloc");
            TangentArgs A = e->tangent_args(e->d_jvp, 1, kTanSunLocal, 0, kJvpSunOffset, sunsky_emitter::kJvpFloats);
            A.st[0] = ts;
            e->stage_tangent(A, st);
            e->jvp_key = key;
            e->jvp_rev = e->rev;
        }
        const float* jvp = e->d_jvp;
        const float *x = wi.x, *y = wi.y, *z = wi.z;
        float sign = -1.f;
        if (!spec) {
            void* args[] = {&lc.K, &jvp, &x, &y, &z, &active, &n, &out, &d_out, &ostride, &sign};
            launch(e->mod->jvp_rgb, grid_for(e->mod, K_EVAL_RGB_V1, n), st, args);
        } else {
            int nl = nlam;
            void* args[] = {&lc.K, &jvp, &x, &y, &z, &lam, &lstride, &nl, &active, &n, &out, &d_out, &ostride, &sign};
            launch(e->mod->jvp_spec, grid_for(e->mod, K_EVAL_SPEC_RAYS_V1, n), st, args);
        }
        e->ad_end(st);
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
            float* d = nullptr;
            hip_check(hipMalloc(&d, sizeof(float) * total), "hipMalloc");
            TangentArgs A = e->tangent_args(d, 1, kTanSunLocal, 0, kJvpSunOffset, total);
            A.st[0] = e->model->tangent_stage(param, tangent, tangent_count);
            e->stage_tangent(A, nullptr);
            hipError_t rc = hipMemcpy(v.data(), d, sizeof(float) * total, hipMemcpyDeviceToHost);
            (void)hipFree(d);
            hip_check(rc, "hipMemcpy");
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
    if (spec && (!lam || nlam < 1 || nlam > kMaxLambdaPerRay))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "spectral eval needs 1..16 wavelength planes");
    const size_t nout = spec ? (size_t)nlam : 3;
    if (!wi.x || !wi.y || !wi.z || !d_out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / cotangent pointer");
    if (nout > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    if (spec && nlam > 1 && lstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "wl_stride < n");
    return guarded([&] {
        Launcher lc(e, stream);
        // basis tangents: turbidity, albedo (all channels at once: channel c's tables depend on
        // albedo[c] only, so the all-ones tangent is the diagonal), sun_direction x / y / z
        const SunskyModel& M = *e->model;
        const int nch = M.nch();
        // 6 workgroups per CU (the RGB kernel holds 3 per CU at a time, 134 VGPRs): few per-block
        // partials, so the one-workgroup reduce below stays short (16384 partials took 0.3 ms)
        const unsigned grid = (unsigned)std::max<size_t>(
            1, std::min<size_t>((n + kBlock - 1) / kBlock, (size_t)e->mod->cu_count * 6));
        hipStream_t st = lc.s;
        const bool stage = !e->d_vjp || e->vjp_rev != e->rev;
        const bool had_ad = e->ad_done != nullptr;
        e->ad_begin(st);   // ordered after the previous AD call (d_vjp / d_partials readers), any stream
        if (e->partials_cap < grid) {
            // the host frees the old partials only once the previous AD call is done with them
            if (had_ad) hip_check(hipEventSynchronize(e->ad_done), "hipEventSynchronize");
            if (e->d_partials) hip_check(hipFree(e->d_partials), "hipFree");
            e->d_partials = nullptr;
            hip_check(hipMalloc(&e->d_partials, sizeof(float) * 16 * grid), "hipMalloc");
            e->partials_cap = grid;
        }
        if (stage) {   // the 5 basis tangents, staged on the device (sunsky_stage_tangent)
            if (!e->d_vjp) hip_check(hipMalloc(&e->d_vjp, sizeof(float) * sunsky_emitter::kVjpFloats), "hipMalloc");
            const int nb = M.active_record() ? 2 : kVjpBases;   // sun_direction is not exposed in time mode
            TangentArgs A = e->tangent_args(e->d_vjp, nb, kVjpSunLocal, 2, kVjpSunOffset, sunsky_emitter::kVjpFloats);
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
        const float* vjp = e->d_vjp;
        float* partials = e->d_partials;
        const float *x = wi.x, *y = wi.y, *z = wi.z;
        float sign = -1.f;
        if (!spec) {
            void* args[] = {&lc.K, &vjp, &x, &y, &z, &active, &n, &d_out, &ostride, &sign, &partials};
            launch(e->mod->vjp_rgb, grid, st, args);
        } else {
            int nl = nlam;
            void* args[] = {&lc.K, &vjp, &x, &y, &z, &lam, &lstride, &nl, &active, &n, &d_out, &ostride, &sign, &partials};
            launch(e->mod->vjp_spec, grid, st, args);
        }
        unsigned nb = grid;
        void* rargs[] = {&partials, &nb, &grad};
        launch(e->mod->grad_reduce, 1, st, rargs);
        e->ad_end(st);
    });
}

// d eval / d wi: argument checks shared by the two calls (sunsky_eval_jvp's rules)
static int dir_ad_check(const sunsky_emitter* e, sunsky_vec3_in wi, const float* lam, int nlam, size_t lstride,
                        size_t n, bool planes_ok, size_t ostride) {
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    const bool spec = e->kargs.variant == kSpectral;
    // an empty batch has no planes to point to (as sunsky_eval_jvp): only the count is checked then
    if (spec && ((n && !lam) || nlam < 1 || nlam > kMaxLambdaPerRay))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "spectral eval needs 1..16 wavelength planes");
    const size_t nout = spec ? (size_t)nlam : 3;
    if (n && (!wi.x || !wi.y || !wi.z || !planes_ok))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / tangent / output pointer");
    if (n && nout > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    if (n && spec && nlam > 1 && lstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "wl_stride < n");
    return SUNSKY_OK;
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
            launch(e->mod->jvp_dir_rgb, grid_for(e->mod, K_EVAL_RGB_V1, n), lc.s, args);
        } else {
            int nl = nlam;
            void* args[] = {&lc.K, &x, &y, &z, &dx, &dy, &dz, &lam, &lstride, &nl, &active, &n, &out, &d_out, &ostride, &sign};
            launch(e->mod->jvp_dir_spec, grid_for(e->mod, K_EVAL_SPEC_RAYS_V1, n), lc.s, args);
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
            launch(e->mod->vjp_dir_rgb, grid_for(e->mod, K_EVAL_RGB_V1, n), lc.s, args);
        } else {
            int nl = nlam;
            void* args[] = {&lc.K, &x, &y, &z, &lam, &lstride, &nl, &active, &n, &d_out, &ostride, &gx, &gy, &gz, &sign};
            launch(e->mod->vjp_dir_spec, grid_for(e->mod, K_EVAL_SPEC_RAYS_V1, n), lc.s, args);
        }
    });
}

int sunsky_bake_latlong(const sunsky_emitter* e, int width, int height, float theta0, float theta1, float phi0,
                        float phi1, const float* lam_host, int m, float* out, size_t ostride, void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "bake_latlong");
    if (!e) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter");
    if (width < 1 || height < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "image size must be >= 1 x 1");
    if ((int64_t)width * height >= (int64_t)1 << 31) return fail(SUNSKY_ERROR_INVALID_VALUE, "image larger than 2^31 pixels");
    const bool spec = e->kargs.variant == kSpectral;
    if (spec && (!lam_host || m < 1 || m > kMaxBroadcastLambda))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "1..32 wavelengths required for a spectral bake");
    if (!spec && lam_host && m) return fail(SUNSKY_ERROR_INVALID_VALUE, "RGB bake takes no wavelengths");
    const size_t n = (size_t)width * (size_t)height;
    if (!out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null output pointer");
    if (ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < width * height");
    // dr::linspace(start, end, count): step = (end - start) / (count - 1) in fp32
    LatLong G = {width, height, theta0, height > 1 ? (theta1 - theta0) / (float)(height - 1) : 0.f,
                 phi0, width > 1 ? (phi1 - phi0) / (float)(width - 1) : 0.f, nullptr};
    return guarded([&] {
        Launcher lc(e, stream);
        hipStream_t s = lc.s;
        const size_t need = 2 * (size_t)width + 2 * (size_t)height;
        // the angle tables are per emitter: order this bake after the previous one (any
        // stream), so a bake on another stream cannot rewrite them under a running kernel
        const bool had_bake = e->bake_done != nullptr;
        if (!had_bake) hip_check(hipEventCreateWithFlags(&e->bake_done, hipEventDisableTiming), "hipEventCreate");
        else hip_check(hipStreamWaitEvent(s, e->bake_done, 0), "hipStreamWaitEvent");
        if (e->bake_cap < need) {
            // the host frees the old tables only once the previous bake is done with them
            if (had_bake) hip_check(hipEventSynchronize(e->bake_done), "hipEventSynchronize");
            if (e->d_bake) hip_check(hipFree(e->d_bake), "hipFree");
            e->d_bake = nullptr;
            hip_check(hipMalloc(&e->d_bake, sizeof(float) * need), "hipMalloc");
            e->bake_cap = need;
        }
        float* tab = e->d_bake;
        G.tab = tab;
        {
            void* targs[] = {&G, &tab};
            const unsigned tg = (unsigned)((std::max(width, height) + kBlock - 1) / kBlock);
            launch(e->mod->latlong_tables, tg, s, targs);
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
        hip_check(hipEventRecord(e->bake_done, s), "hipEventRecord");
    });
}

// ---------------------------------------------------------------- frame sequences
int sunsky_sun_coordinates(int year, int month, int day, float hour, float minute, float second, float latitude,
                           float longitude, float timezone, float out[3]) {
    if (!out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null output pointer");
    DateTime t;
    t.year = year; t.month = month; t.day = day; t.hour = hour; t.minute = minute; t.second = second;
    Location l;
    l.latitude = latitude; l.longitude = longitude; l.timezone = timezone;
    compute_sun_coordinates(t, l, out);
    return SUNSKY_OK;
}

int sunsky_sequence_create(const sunsky_emitter* e, int count, const float* sun_dirs, const float* turbidity,
                           const float* weights, sunsky_sequence** out) {
    SUNSKY_PHASE("InitScene", "sequence_create");
    if (!e || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null emitter / output pointer");
    *out = nullptr;
    if (count < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "a sequence needs at least one frame (count >= 1)");
    if (!sun_dirs) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sun direction array");
    return guarded([&] {
        std::unique_ptr<sunsky_sequence> q(new sunsky_sequence());
        const SunskyModel& model = *e->model;
        q->kargs = e->kargs;
        q->kargs.sun_table = nullptr;   // no per-frame sun table: the disc lanes lerp the raw dataset
        q->kargs.sun_ld = nullptr;
        q->count = count;
        q->nch = model.nch();
        q->variant = model.variant();
        q->precision = e->precision;
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
        if (e->device < 0) {
            q->h_sun_rad = model.sun_rad_ds();   // prepare_sampling's disc term on the host
            q->h_sun_ld = model.sun_ld();
            q->h_sky_params_ds = model.sky_params_ds();
            q->h_sky_rad_ds = model.sky_rad_ds();
            seq_restage(q.get(), dirs, T, w);
            q->in_dirs = std::move(dirs); q->in_turbidity = std::move(T); q->in_weights = std::move(w);
            *out = q.release();
            return;
        }
        DeviceScope g(e->device);
        q->mod = e->mod;
        // from here on the destructor frees what was allocated
        q->device = e->device;
        const std::vector<float>& su = model.sun_rad_ds();
        const std::vector<float>& ld = model.sun_ld();
        const std::vector<float>& sp = model.sky_params_ds();
        const std::vector<float>& sr = model.sky_rad_ds();
        hip_check(hipMalloc(&q->d_frames, (size_t)count * q->rec_bytes), "hipMalloc");
        hip_check(hipMalloc(&q->d_sun_rad, sizeof(float) * su.size()), "hipMalloc");
        hip_check(hipMalloc(&q->d_sun_ld, sizeof(float) * kNbWavelengths * kNbSunLdParams), "hipMalloc");
        hip_check(hipMalloc(&q->d_state, sizeof(SunskyKArgs)), "hipMalloc");
        hip_check(hipMalloc(&q->d_sky_ds, sizeof(float) * (sp.size() + sr.size())), "hipMalloc");
        hip_check(hipMemcpy(q->d_sun_rad, su.data(), sizeof(float) * su.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemset(q->d_sun_ld, 0, sizeof(float) * kNbWavelengths * kNbSunLdParams), "hipMemset");
        hip_check(hipMemcpy(q->d_sun_ld, ld.data(), sizeof(float) * std::min<size_t>(ld.size(), kNbWavelengths * kNbSunLdParams),
                            hipMemcpyHostToDevice), "hipMemcpy");
        // the raw sky datasets, the sequence's own copy: update restages from it when the parent is gone
        hip_check(hipMemcpy(q->d_sky_ds, sp.data(), sizeof(float) * sp.size(), hipMemcpyHostToDevice), "hipMemcpy");
        hip_check(hipMemcpy(q->d_sky_ds + sp.size(), sr.data(), sizeof(float) * sr.size(), hipMemcpyHostToDevice), "hipMemcpy");
        q->d_sky_params_ds = q->d_sky_ds;
        q->d_sky_rad_ds = q->d_sky_ds + sp.size();
        q->kargs.sun_ld = q->d_sun_ld;
        hip_check(hipMemcpy(q->d_state, &q->kargs, sizeof(SunskyKArgs), hipMemcpyHostToDevice), "hipMemcpy");
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
        std::unique_ptr<DeviceScope> g;
        if (seq->device >= 0) {
            g.reset(new DeviceScope(seq->device));
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // nothing may still read the old records
        }
        seq_restage(seq, dirs, T, w);   // throws with the sequence untouched when a frame is refused
        seq->in_dirs = std::move(dirs); seq->in_turbidity = std::move(T); seq->in_weights = std::move(w);
        // the sampling distribution described the old frames
        seq->samp_nz = seq->samp_nphi = 0;
        seq->irr_nz = seq->irr_nphi = seq->irr_planes = 0;   // and so did the irradiance tables
        seq->irr_grad_ready = false;                         // and what their gradients read (wanted stays)
        if (seq->grad_ready) seq_stage_grad(seq);
    });
}

int sunsky_sequence_prepare_grad(sunsky_sequence* seq) {
    SUNSKY_PHASE("InitScene", "sequence_prepare_grad");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        std::unique_ptr<DeviceScope> g;
        if (seq->device >= 0) {
            g.reset(new DeviceScope(seq->device));
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // nothing may still read the old records
            if (!seq->d_grad_rows) {   // once: the records, the staging scalars, the rows of the largest grid
                seq->grad_max_grid = seq_grad_grid(seq, ~(size_t)0 / 2);
                const size_t rows = (size_t)seq->grad_max_grid * seq_grad_rows_per_block(seq);
                if (!seq->d_grads) hip_check(hipMalloc(&seq->d_grads, (size_t)seq->count * seq_grad_bytes(seq->nch)), "hipMalloc");
                if (!seq->d_grad_stages)
                    hip_check(hipMalloc(&seq->d_grad_stages, sizeof(TangentStage) * (size_t)seq->count), "hipMalloc");
                hip_check(hipMalloc(&seq->d_grad_rows, sizeof(float) * rows * (size_t)seq->count * kSeqGradSums), "hipMalloc");
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
    if (spec && (!lam_host || m < 1 || m > kMaxBroadcastLambda))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "1..32 broadcast wavelengths required for a spectral sequence");
    if (!spec && lam_host && m) return fail(SUNSKY_ERROR_INVALID_VALUE, "an RGB sequence takes no wavelengths");
    if (n == 0) return SUNSKY_OK;
    if (!wi.x || !wi.y || !wi.z) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray pointer");
    if (!d_out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null cotangent (d_out)");
    if ((spec ? m : 3) > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    return guarded([&] {
        seq->require_grad();   // first: the message names the missing call on any sequence
        seq->require_device();
        if (!grad_weight && !grad_turbidity && !grad_sun_dir) return;
        DeviceScope g(seq->device);
        hipStream_t s = (hipStream_t)stream;
        const unsigned grid = seq_grad_grid(seq, n);   // <= grad_max_grid: the workspace holds its rows
        const bool lds = seq->count <= kSeqGradLdsFrames;
        const SunskyKArgs* K = seq->d_state;
        SeqArgs A = seq->args();
        SeqGradArgs G = {seq->d_grads, d_out, ostride, seq->d_grad_rows, lds ? 1 : 0, 0};
        const unsigned dyn = lds ? (unsigned)(sizeof(float) * (kBlock / 64) * (size_t)seq->count * kSeqGradSums) : 0u;
        // reference arithmetic whatever the sequence's precision: both names run the same body
        const auto& fns = seq->mod->fn[seq->xform_form()][SUNSKY_PRECISION_REFERENCE];
        if (!spec) {
            void* args[] = {&K, &A, &G, (void*)&wi.x, (void*)&wi.y, (void*)&wi.z, &active, &n};
            launch(fns[K_SEQUENCE_EVAL_VJP_RGB], grid, s, args, dyn);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&K, &A, &G, &L, (void*)&wi.x, (void*)&wi.y, (void*)&wi.z, &active, &n};
            launch(fns[K_SEQUENCE_EVAL_VJP_SPEC], grid, s, args, dyn);
        }
        const float* rows = seq->d_grad_rows;
        unsigned nrows = grid * (unsigned)seq_grad_rows_per_block(seq);
        int count = seq->count;
        void* rargs[] = {(void*)&rows, &nrows, &count, &grad_weight, &grad_turbidity, &grad_sun_dir};
        hip_check(hipModuleLaunchKernel(seq->mod->sequence_grad_reduce, (unsigned)std::min(count, 65535), 1, 1,
                                        kSeqGradReduceBlock, 1, 1, 0, s, rargs, nullptr),
                  "hipModuleLaunchKernel(sunsky_sequence_grad_reduce)");
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
    if (spec && (!lam_host || m < 1 || m > kMaxBroadcastLambda))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "1..32 broadcast wavelengths required for a spectral sequence");
    if (!spec && lam_host && m) return fail(SUNSKY_ERROR_INVALID_VALUE, "an RGB sequence takes no wavelengths");
    if (n == 0) return SUNSKY_OK;
    if (!w.x || !w.y || !w.z || !out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null ray / output pointer");
    if ((spec ? m : 3) > 1 && ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < n");
    return guarded([&] {
        seq->require_device();
        DeviceScope g(seq->device);
        const SunskyKArgs* K = seq->d_state;
        SeqArgs A = seq->args();
        if (!spec) {
            void* args[] = {&K, &A, (void*)&w.x, (void*)&w.y, (void*)&w.z, &active, &n, &out, &ostride};
            run_kernel(seq->mod, seq->xform_form(), seq->precision, K_SEQUENCE_EVAL_RGB, n, args, (hipStream_t)stream);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&K, &A, &L, (void*)&w.x, (void*)&w.y, (void*)&w.z, &active, &n, &out, &ostride};
            run_kernel(seq->mod, seq->xform_form(), seq->precision, K_SEQUENCE_EVAL_SPEC, n, args, (hipStream_t)stream);
        }
    });
}

int sunsky_sequence_bake_latlong(const sunsky_sequence* seq, int width, int height, float theta0, float theta1,
                                 float phi0, float phi1, const float* lam_host, int m, float* out, size_t ostride,
                                 void* stream) {
    SUNSKY_PHASE("EndpointEvaluate", "sequence_bake_latlong");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    if (width < 1 || height < 1) return fail(SUNSKY_ERROR_INVALID_VALUE, "image size must be >= 1 x 1");
    if ((int64_t)width * height >= (int64_t)1 << 31) return fail(SUNSKY_ERROR_INVALID_VALUE, "image larger than 2^31 pixels");
    const bool spec = seq->variant == kSpectral;
    if (spec && (!lam_host || m < 1 || m > kMaxBroadcastLambda))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "1..32 wavelengths required for a spectral bake");
    if (!spec && lam_host && m) return fail(SUNSKY_ERROR_INVALID_VALUE, "RGB bake takes no wavelengths");
    const size_t n = (size_t)width * (size_t)height;
    if (!out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null output pointer");
    if (ostride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "out_stride < width * height");
    LatLong G = {width, height, theta0, height > 1 ? (theta1 - theta0) / (float)(height - 1) : 0.f,
                 phi0, width > 1 ? (phi1 - phi0) / (float)(width - 1) : 0.f, nullptr};
    return guarded([&] {
        seq->require_device();
        DeviceScope g(seq->device);
        hipStream_t s = (hipStream_t)stream;
        // the angle tables are per sequence, ordered between bakes as sunsky_bake_latlong's
        const size_t need = 2 * (size_t)width + 2 * (size_t)height;
        const bool had_bake = seq->bake_done != nullptr;
        if (!had_bake) hip_check(hipEventCreateWithFlags(&seq->bake_done, hipEventDisableTiming), "hipEventCreate");
        else hip_check(hipStreamWaitEvent(s, seq->bake_done, 0), "hipStreamWaitEvent");
        if (seq->bake_cap < need) {
            if (had_bake) hip_check(hipEventSynchronize(seq->bake_done), "hipEventSynchronize");
            if (seq->d_bake) hip_check(hipFree(seq->d_bake), "hipFree");
            seq->d_bake = nullptr;
            seq->bake_cap = 0;
            hip_check(hipMalloc(&seq->d_bake, sizeof(float) * need), "hipMalloc");
            seq->bake_cap = need;
        }
        float* tab = seq->d_bake;
        G.tab = tab;
        {
            void* targs[] = {&G, &tab};
            const unsigned tg = (unsigned)((std::max(width, height) + kBlock - 1) / kBlock);
            launch(seq->mod->latlong_tables, tg, s, targs);
        }
        const SunskyKArgs* K = seq->d_state;
        SeqArgs A = seq->args();
        if (!spec) {
            void* args[] = {&K, &A, &G, &out, &ostride};
            run_kernel(seq->mod, seq->xform_form(), seq->precision, K_SEQUENCE_BAKE_RGB, n, args, s);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&K, &A, &G, &L, &out, &ostride};
            run_kernel(seq->mod, seq->xform_form(), seq->precision, K_SEQUENCE_BAKE_SPEC, n, args, s);
        }
        hip_check(hipEventRecord(seq->bake_done, s), "hipEventRecord");
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
        if (seq->d_samp) hip_check(hipFree(seq->d_samp), "hipFree");
        seq->d_samp = nullptr;
        hip_check(hipMalloc(&seq->d_samp, sizeof(float) * lay.total), "hipMalloc");
        hip_check(hipMemset(seq->d_samp, 0, sizeof(float) * lay.total), "hipMemset");
        SeqTableArgs T;
        std::memset(&T, 0, sizeof(T));
        T.f = seq->d_samp + lay.f;
        T.B = seq->d_samp + lay.suns;   // B_k rests where the sun records go
        std::memcpy(T.cie_y, seq->cie_y, sizeof(T.cie_y));
        T.nz = n_z;
        T.nphi = n_phi;
        const SunskyKArgs* K = seq->d_state;
        SeqArgs A = seq->args();
        void* args[] = {&K, &A, &T};
        const unsigned grid = (unsigned)std::min<size_t>((cells + kBlock - 1) / kBlock, (size_t)seq->mod->cu_count * 64);
        launch(seq->mod->sequence_table, grid, nullptr, args);
        hip_check(hipModuleLaunchKernel(seq->mod->sequence_suns, (unsigned)std::min(seq->count, 65535), 1, 1, 64, 1, 1, 0,
                                        nullptr, args, nullptr), "hipModuleLaunchKernel(sunsky_sequence_suns)");
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
        hip_check(hipMemcpy(seq->d_samp, block.data(), sizeof(float) * lay.total, hipMemcpyHostToDevice), "hipMemcpy");
        // q_k into the records (SeqFrame::pad[0]): the sample kernels read it beside the header
        hip_check(hipMemcpy(seq->d_frames, seq->records.data(), seq->records.size(), hipMemcpyHostToDevice), "hipMemcpy");
        SeqSampling& s = seq->samp;
        s.f = seq->d_samp + lay.f;
        s.row_cdf = seq->d_samp + lay.row_cdf;
        s.cell_cdf = seq->d_samp + lay.cell_cdf;
        s.frame_cdf = seq->d_samp + lay.frame_cdf;
        s.suns = seq->d_samp + lay.suns;
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
    if (spec && (!lam_host || m < 1 || m > kMaxBroadcastLambda))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "1..32 broadcast wavelengths required for a spectral sequence");
    if (!spec && lam_host && m) return fail(SUNSKY_ERROR_INVALID_VALUE, "an RGB sequence takes no wavelengths");
    if (n == 0) return SUNSKY_OK;
    if (!ux || !uy || !ds_d.x || !ds_d.y || !ds_d.z || !ds_pdf || !weight)
        return fail(SUNSKY_ERROR_INVALID_VALUE, "null sample / output pointer");
    if ((spec ? m : 3) > 1 && wstride < n) return fail(SUNSKY_ERROR_INVALID_VALUE, "weight_stride < n");
    if ((it_p.x != nullptr) != (it_p.y != nullptr) || (it_p.x != nullptr) != (it_p.z != nullptr))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "it_p must be all-NULL or all-set");
    if ((ds_p.x != nullptr) != (ds_p.y != nullptr) || (ds_p.x != nullptr) != (ds_p.z != nullptr))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "ds_p must be all-NULL or all-set");
    return guarded([&] {
        seq->require_sampling();   // first: the message names the missing call on any sequence
        seq->require_device();
        DeviceScope g(seq->device);
        const SunskyKArgs* K = seq->d_state;
        SeqArgs A = seq->args();
        SeqSampling S = seq->samp;
        SeqSampleIO io = {ux, uy, it_p.x, it_p.y, it_p.z, active, ds_d.x, ds_d.y, ds_d.z, ds_pdf, ds_dist,
                          ds_p.x, ds_p.y, ds_p.z, weight, wstride};
        if (!spec) {
            void* args[] = {&K, &A, &S, &io, &n};
            run_kernel(seq->mod, seq->xform_form(), seq->precision, K_SEQUENCE_SAMPLE_RGB, n, args, (hipStream_t)stream);
        } else {
            LambdaSet L = make_lambda_set(lam_host, m);
            void* args[] = {&K, &A, &S, &L, &io, &n};
            run_kernel(seq->mod, seq->xform_form(), seq->precision, K_SEQUENCE_SAMPLE_SPEC, n, args, (hipStream_t)stream);
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
        seq->require_device();
        DeviceScope g(seq->device);
        const SunskyKArgs* K = seq->d_state;
        SeqSampling S = seq->samp;
        int count = seq->count;
        void* args[] = {&K, &S, &count, (void*)&d.x, (void*)&d.y, (void*)&d.z, &active, &n, &pdf};
        run_kernel(seq->mod, seq->xform_form(), seq->precision, K_SEQUENCE_PDF, n, args, (hipStream_t)stream);
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
        };
        seq->irr_grad_ready = false;
        if (seq->device < 0) {
            seq_irradiance_host(seq, n_z, n_phi, T.L, planes, T.sin2_half_ap, sky, flux);
            accept();
            return;
        }
        DeviceScope g(seq->device);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // nothing may still read the old image
        seq->irr_nz = seq->irr_nphi = seq->irr_planes = 0;
        if (seq->d_irr) hip_check(hipFree(seq->d_irr), "hipFree");
        seq->d_irr = nullptr;
        // the image's allocation first holds the two tables the kernels write: a record has 3 floats
        // more than planes, so it is never smaller
        const size_t rec = (size_t)seq_irr_record(planes);
        const size_t image_cap = (cells + (size_t)count) * rec;
        static_assert(sizeof(int) == sizeof(float), "the suns' columns lie behind the image");
        hip_check(hipMalloc(&seq->d_irr, sizeof(float) * (image_cap + (size_t)count)), "hipMalloc");
        T.sky = seq->d_irr;
        T.flux = seq->d_irr + sky.size();
        const SunskyKArgs* K = seq->d_state;
        SeqArgs A = seq->args();
        void* args[] = {&K, &A, &T};
        const unsigned grid = (unsigned)std::min<size_t>((cells + kBlock - 1) / kBlock, (size_t)seq->mod->cu_count * 64);
        launch(seq->mod->irradiance_table, grid, nullptr, args);
        hip_check(hipModuleLaunchKernel(seq->mod->irradiance_flux, (unsigned)std::min(count, 65535), 1, 1, 64, 1, 1, 0,
                                        nullptr, args, nullptr), "hipModuleLaunchKernel(sunsky_sequence_irradiance_flux)");
        hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
        hip_check(hipMemcpy(sky.data(), T.sky, sizeof(float) * sky.size(), hipMemcpyDeviceToHost), "hipMemcpy");
        hip_check(hipMemcpy(flux.data(), T.flux, sizeof(float) * flux.size(), hipMemcpyDeviceToHost), "hipMemcpy");
        std::vector<int> kept;
        const int nsuns = seq_irradiance_image(seq, n_z, n_phi, planes, omega, sky, flux, image, kept);
        hip_check(hipMemcpy(seq->d_irr, image.data(), sizeof(float) * image.size(), hipMemcpyHostToDevice), "hipMemcpy");
        seq->irr = SeqIrradiance{seq->d_irr, seq->d_irr + cells * rec, n_z, n_phi, nsuns, planes};
        for (int& k : kept) k = cols[(size_t)k];   // the image's suns' columns, in its order
        seq->d_irr_sun_cols = reinterpret_cast<const int*>(seq->d_irr + image_cap);
        if (nsuns)
            hip_check(hipMemcpy(seq->d_irr + image_cap, kept.data(), sizeof(int) * kept.size(), hipMemcpyHostToDevice),
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
        seq->require_device();
        if (seq->irr_planes > 1 && ostride < n) throw std::invalid_argument("out_stride < n");
        DeviceScope g(seq->device);
        const SunskyKArgs* K = seq->d_state;
        SeqIrradiance S = seq->irr;
        void* args[] = {&K, &S, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &out, &ostride};
        run_kernel(seq->mod, seq->xform_form(), seq->precision,
                   seq->variant == kSpectral ? K_SEQUENCE_IRRADIANCE_SPEC : K_SEQUENCE_IRRADIANCE_RGB, n, args,
                   (hipStream_t)stream);
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
        seq->require_device();
        DeviceScope g(seq->device);
        const SunskyKArgs* K = seq->d_state;
        SeqIrradiance S = seq->irr;
        SeqIrrHorizon Z = {horizon, seq->d_irr_sun_cols, hstride, n_sectors, seq->irr_nphi / n_sectors,
                           n_profiles == 1 ? 0 : 1, 0};
        void* args[] = {&K, &S, &Z, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &out, &ostride};
        run_kernel(seq->mod, seq->xform_form(), seq->precision,
                   seq->variant == kSpectral ? K_SEQUENCE_IRRADIANCE_HORIZON_SPEC : K_SEQUENCE_IRRADIANCE_HORIZON_RGB, n,
                   args, (hipStream_t)stream);
    });
}

int sunsky_sequence_prepare_irradiance_grad(sunsky_sequence* seq) {
    SUNSKY_PHASE("InitScene", "sequence_prepare_irradiance_grad");
    if (!seq) return fail(SUNSKY_ERROR_INVALID_VALUE, "null sequence");
    return guarded([&] {
        seq->require_irradiance();
        std::unique_ptr<DeviceScope> g;
        if (seq->device >= 0) {
            g.reset(new DeviceScope(seq->device));
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // nothing may still use the old workspace
        }
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
    if ((grad_normal.x != nullptr) != (grad_normal.y != nullptr) || (grad_normal.x != nullptr) != (grad_normal.z != nullptr))
        return fail(SUNSKY_ERROR_INVALID_VALUE, "grad_normal must be all-NULL or all-set");
    if (n > 0xffffff00ull) return fail(SUNSKY_ERROR_INVALID_VALUE, "more than 2^32 - 256 receivers");
    return guarded([&] {
        seq->require_irradiance_grad();   // first: the message names the missing call on any sequence
        seq->require_device();
        if (seq->irr_planes > 1 && d_stride < n) throw std::invalid_argument("d_stride < n");
        DeviceScope g(seq->device);
        const SunskyKArgs* K = seq->d_state;
        SeqIrradiance S = seq->irr;
        const bool spec = seq->variant == kSpectral;
        const int form = seq->xform_form();
        hipStream_t s = (hipStream_t)stream;
        if (grad_normal.x) {
            void* args[] = {&K, &S, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n, &d_out, &d_stride,
                            (void*)&grad_normal.x, (void*)&grad_normal.y, (void*)&grad_normal.z};
            run_kernel(seq->mod, form, seq->precision,
                       spec ? K_SEQUENCE_IRRADIANCE_VJP_NORMAL_SPEC : K_SEQUENCE_IRRADIANCE_VJP_NORMAL_RGB, n, args, s);
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
            void* args[] = {&K, &S, &G, (void*)&nrm.x, (void*)&nrm.y, (void*)&nrm.z, &active, &n};
            run_kernel(seq->mod, form, seq->precision, K_SEQUENCE_IRRADIANCE_ADJOINT,
                       (size_t)shape.slices * tiles * passes * kBlock, args, s);
        }
        SeqArgs A = seq->args();
        LambdaSet L = seq->irr_L;
        for (int phase = shape.slices > 1 ? 0 : 1; phase < 2; ++phase) {
            void* args[] = {&K, &A, &S, &G, &L, &phase, &grad_weight};
            run_kernel(seq->mod, form, seq->precision, K_SEQUENCE_IRRADIANCE_GRAD_FOLD,
                       phase == 0 ? (size_t)seq->irr_planes * entries : (size_t)seq->count * kBlock, args, s);
        }
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

int sunsky_array_from_file(const char* path, int file_dtype, double* out, size_t cap, size_t* count, uint64_t* shape,
                           int* ndims) {
    if (!path || !count) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    Table t;
    std::string err;
    if (!read_array_file(path, file_dtype, &t, &err))
        return fail(err.find("does not exist") != std::string::npos ? SUNSKY_ERROR_FILE : SUNSKY_ERROR_FORMAT, err);
    *count = t.size();
    if (out) std::memcpy(out, t.data.data(), sizeof(double) * std::min(cap, t.size()));
    if (ndims) *ndims = (int)t.shape.size();
    if (shape)
        for (size_t i = 0; i < t.shape.size() && i < 16; ++i) shape[i] = t.shape[i];
    return SUNSKY_OK;
}

int sunsky_array_to_file(const char* path, const float* data, size_t count, const uint64_t* shape, int ndims) {
    if (!path || (!data && count)) return fail(SUNSKY_ERROR_INVALID_VALUE, "null argument");
    std::vector<size_t> sh;
    for (int i = 0; i < ndims; ++i) sh.push_back((size_t)shape[i]);
    std::string err;
    if (!write_array_file(path, data, count, sh.empty() ? nullptr : sh.data(), (int)sh.size(), &err))
        return fail(SUNSKY_ERROR_FILE, err);
    return SUNSKY_OK;
}

const char* plugin_name(void) { return "sunsky"; }
const char* plugin_descr(void) { return "Sun and Sky dome background emitter (MI355X)"; }

int sunsky_hosek_sun_rad(const char* dataset_path, double turbidity, double wavelength, double elevation,
                         double gamma, double* out) {
    if (!out) return fail(SUNSKY_ERROR_INVALID_VALUE, "null output pointer");
    return guarded([&] {
        std::string ds = dataset_path && *dataset_path ? std::string(dataset_path) : default_pack_path();
        *out = hosek_solar_radiance(ds, turbidity, wavelength, elevation, gamma);
    });
}

int sunsky_default_dataset_path(char* buf, size_t cap) {
    if (!buf || !cap) return fail(SUNSKY_ERROR_INVALID_VALUE, "null buffer");
    std::snprintf(buf, cap, "%s", default_pack_path().c_str());
    return SUNSKY_OK;
}

}  // extern "C"
