// sunsky_launch.cpp -- the code objects, the per-device kernel table and the launch helpers
// (sunsky_launch.h).
#include "sunsky_launch.h"

#include <dlfcn.h>
#include <sys/stat.h>

#include <map>
#include <mutex>

namespace sunsky {
namespace capi {

std::string& last_error() {
    thread_local std::string g_error;
    return g_error;
}

namespace {

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

std::mutex g_module_mutex;
std::map<int, DeviceModule*> g_modules;

// The 11-node spectral kernel with more than one step per lane (configs[4]'s 64M directions
// per GPU): unused dynamic LDS that holds it to 5 workgroups (5 waves/SIMD) per CU.  Fewer
// concurrent 11-plane write streams per CU write HBM faster there: 64M x 11 cold, 774 ->
// 750 us at 5 and 745 us at 4 workgroups per CU, 806 us at 2; at one step per lane (16M)
// neutral (profiles/r06_v8_nodes_occupancy_cold.log, r06_v7_ab_nodes_lds_cap.log).
constexpr unsigned kNodesLdsCap = 32000;

}  // namespace

std::string default_pack_path() {
    if (const char* env = std::getenv("SUNSKY_AMD_DATASET")) return env;
    std::string d = library_dir();
    for (const char* rel : {"/sunsky_datasets.pack", "/../data/sunsky_datasets.pack", "/data/sunsky_datasets.pack"})
        if (file_exists(d + rel)) return d + rel;
    return d + "/../data/sunsky_datasets.pack";
}

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
                const bool plain = kKernels[k].forms == PLAIN;   // the general object's one function, four times
                hipModule_t mod = id && !plain ? m->module_ident : m->module;
                const std::string name = kKernels[k].name;
                const std::string prec = plain ? "" : p == SUNSKY_PRECISION_FAST ? "_fast" : "_ref";
                get(&m->fn[id][p][k], mod, name + prec);
                if (kKernels[k].dir_form) get(&m->fn_dir[id][p][k], mod, name + "_dir" + prec);
            }
    hip_check(hipDeviceGetAttribute(&m->cu_count, hipDeviceAttributeMultiprocessorCount, dev),
              "hipDeviceGetAttribute");
    DeviceModule* raw = m.release();
    g_modules[dev] = raw;
    return raw;
}

unsigned grid_for(const DeviceModule* m, KernelId k, size_t work_items, bool tunable) {
    static const int env = [] {
        const char* e = std::getenv("SUNSKY_AMD_BLOCKS_PER_CU");
        return e ? std::max(1, std::atoi(e)) : 0;
    }();
    size_t need = (work_items + kBlock - 1) / kBlock;
    size_t cap = (size_t)m->cu_count * (size_t)(env && tunable ? env : kKernels[k].blocks_per_cu);
    return (unsigned)std::max<size_t>(1, std::min(need, cap));
}

void launch(hipFunction_t f, unsigned grid, unsigned block, hipStream_t s, void** args, unsigned dyn_lds) {
    hip_check(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, dyn_lds, s, args, nullptr), "hipModuleLaunchKernel");
}

void run_kernel(const DeviceModule* mod, int form, int precision, KernelId k, size_t n, void** args, hipStream_t s,
                bool dir) {
    const size_t per = (size_t)kKernels[k].per_item, items = (n + per - 1) / per;
    const unsigned grid = grid_for(mod, k, items);
    const bool multi_step = items > (size_t)grid * kBlock;
    const auto& fns = dir ? mod->fn_dir : mod->fn;
    launch(fns[form][precision][k], grid, kBlock, s, args, k == K_EVAL_SPEC_NODES_V4 && multi_step ? kNodesLdsCap : 0u);
}

size_t vec4_count(size_t n, std::initializer_list<const void*> planes, std::initializer_list<size_t> strides,
                  const uint8_t* active) {
    bool vec = n >= 4 && (!active || ((uintptr_t)active & 3u) == 0);
    for (const void* p : planes) vec = vec && ((uintptr_t)p & 15u) == 0;
    for (size_t s : strides) vec = vec && (s % 4) == 0;
    return vec ? (n & ~(size_t)3) : 0;
}

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

}  // namespace capi
}  // namespace sunsky
