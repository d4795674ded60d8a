// sunsky_kernel_args.h -- the structs that kernels take by value (beside SunskyKArgs,
// sunsky_types.h, and TangentArgs, sunsky_staging.h): one definition, read by the kernels
// (sunsky_kernels.hip), by the C-ABI layer that fills them (sunsky_capi.cpp) and by
// tools/kbench.cpp.  The sizes are pinned so that the host compiler and the device
// compiler each check the layout they pass / read.
#pragma once
#include <cstddef>

#include "sunsky_staging.h"
#include "sunsky_types.h"

namespace sunsky {

// eval_spectral_broadcast / spectral bake: one wavelength set for every direction.
// Wavelength k maps to channels (lo[k], lo[k] + 1, f[k]), computed on the host.
struct LambdaSet {
    int m;
    int lo[kMaxBroadcastLambda];
    float f[kMaxBroadcastLambda];   // < 0: invalid wavelength (output 0)
};
static_assert(sizeof(LambdaSet) == 4 + 8 * kMaxBroadcastLambda, "LambdaSet layout");

// The rough conductor of the glossy caller (alpha_v after the IOR so the isotropic
// layout's offsets stay)
struct ConductorArgs {
    int type;            // 0 Beckmann, 1 GGX (MicrofacetType)
    float alpha_u;       // roughness along the frame's s (microfacet.h m_alpha_u)
    float eta[4], k[4];  // complex IOR per RGB channel (spectral: eta[0], k[0] for every wavelength)
    float alpha_v;       // roughness along t (= alpha_u: isotropic)
};
static_assert(sizeof(ConductorArgs) == 44 && offsetof(ConductorArgs, alpha_v) == 40, "ConductorArgs layout");

// bake_latlong: the image grid and its angle tables (cos / sin phi per column, sin / cos
// theta per row, written by sunsky_latlong_tables)
struct LatLong { int w, h; float theta0, dtheta, phi0, dphi; const float* tab; };
static_assert(sizeof(LatLong) == 32, "LatLong layout");

// sunsky_stage_radiance (parameters_changed on the device)
struct StageArgs {
    SunskyKArgs* state;            // the emitter's device state (sky[], fsky[] written)
    float* sun_table;              // its turbidity-lerped sun table (written)
    const float* sky_params_ds;    // (10 T, 2 albedo, 6 ctrl, nch, 9)
    const float* sky_rad_ds;       // (10, 2, 6, nch)
    const float* sun_rad_ds;       // (10, sun_block)
    RadianceStage rs;
    float albedo[kNbWavelengths];
    int nch, variant, sun_block;
    float sky_scale;
};
static_assert(sizeof(StageArgs) == 40 + sizeof(RadianceStage) + 4 * kNbWavelengths + 16, "StageArgs layout");

constexpr int kQuadBlock = 256;    // one quadrature row per workgroup, one point per thread

// sunsky_stage_quad_points / sunsky_stage_quad_finish (the JIT sampling weight)
struct QuadArgs {
    SunskyKArgs* state;
    const float* qx;               // 200 Gauss-Legendre nodes / weights (fp32)
    const float* qw;
    float* rows;                   // [2][nq][nch] row sums (sky, sun)
    int nq, nch;
    float cie_y[kNbWavelengths];
    float sky_scale, sun_scale;
    int* status;                   // set to 1 by a rejected staging (negative wavelength-distribution entry)
};
static_assert(sizeof(QuadArgs) == 104 && offsetof(QuadArgs, status) == 96, "QuadArgs layout");

}  // namespace sunsky
