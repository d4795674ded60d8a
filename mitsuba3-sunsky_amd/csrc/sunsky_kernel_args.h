// sunsky_kernel_args.h -- the structs that kernels take by value (beside SunskyKArgs,
// sunsky_types.h, and TangentArgs, sunsky_staging.h): one definition, read by the kernels
// (sunsky_kernels.hip and its parts, kernels/*.h), by the C-ABI layer that fills them (sunsky_capi_*.cpp) and by
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

// ---------------------------------------------------------------- frame sequences
// One frame of a sunsky_sequence in device memory (NCH = 3 RGB, 11 spectral): what differs
// between the frames of one emitter.  The host fills the header (and zeroes the channels);
// sunsky_stage_sequence writes the channels in place from the header's RadianceStage scalars
// (host-only sequences run the same functions on the host).  The accumulate kernels read a
// record with one address per wave: every block is 16-byte aligned for wide scalar loads.
template <int NCH>
struct alignas(16) SeqFrame {
    float sun_n[3];            // local sun direction (m_local_sun_frame.n of the frame's emitter)
    float weight;
    float t_rem;               // turbidity lerp scalars (RadianceStage): the disc lanes' sun_param
    int t_low, t_high;
    float turbidity;
    float x;                   // cbrt(2 eta / pi) of the frame's sun elevation (staging only)
    int in_range;              // 0 <= eta <= pi / 2 (staging only)
    float pad[2];
    FastChannel fast[NCH];     // FAST kernels
    SkyChannel sky[NCH];       // reference kernels, get_frame
};
constexpr size_t kSeqFrameHeader = 48;
static_assert(sizeof(SkyChannel) == 64, "SkyChannel record stride");
static_assert(sizeof(SeqFrame<3>) == kSeqFrameHeader + 3 * 112 && sizeof(SeqFrame<kNbWavelengths>) == kSeqFrameHeader + 11 * 112,
              "SeqFrame layout");
static_assert(offsetof(SeqFrame<3>, weight) == 12 && offsetof(SeqFrame<3>, t_rem) == 16 &&
              offsetof(SeqFrame<3>, x) == 32 && offsetof(SeqFrame<3>, fast) == kSeqFrameHeader &&
              offsetof(SeqFrame<3>, sky) == kSeqFrameHeader + 3 * 48 &&
              offsetof(SeqFrame<kNbWavelengths>, sky) == kSeqFrameHeader + 11 * 48, "SeqFrame layout");

// sunsky_stage_sequence: one workgroup per frame
struct SeqStageArgs {
    void* frames;                  // SeqFrame<nch>[count], headers filled
    const float* sky_params_ds;    // the raw sky datasets: the sequence's own device copy (create and update)
    const float* sky_rad_ds;
    float albedo[kNbWavelengths];
    int nch, variant, count;
    float sky_scale;
};
static_assert(sizeof(SeqStageArgs) == 24 + 4 * kNbWavelengths + 16 + 4, "SeqStageArgs layout");

// The accumulate kernels' view of a sequence
struct SeqArgs {
    const void* frames;            // SeqFrame<nch>[count]
    const float* sun_rad_ds;       // raw sun dataset (10 turbidities x sun block), device
    int count, sun_block;
};
static_assert(sizeof(SeqArgs) == 24, "SeqArgs layout");

// ---------------------------------------------------------------- sequence gradients
// One frame's gradient record (sunsky_sequence_prepare_grad; NCH = 3 RGB, 11 spectral): the
// tangents of the frame's staged tables that sunsky_sequence_eval_vjp contracts per ray.  The
// host fills dlocal / deta (tangent_stage_for) and sunsky_stage_sequence_grad writes the two sky
// blocks in place (tangent_value, fp64).  Every block starts on 16 bytes: the kernels read a
// record with one address per wave, as they read SeqFrame.
constexpr int seq_grad_block(int nch) { return (nch * 10 + 3) & ~3; }   // 32 RGB, 112 spectral
template <int NCH>
struct alignas(16) SeqGradFrame {
    float dsky_T[seq_grad_block(NCH)];     // d{A..I, rad} / dT per channel (c x 10 + q), floor(T) constant
    float dsky_eta[seq_grad_block(NCH)];   // ... / d eta: the unit-elevation tangent
    float dlocal[3][3];                    // d local sun direction / d s[a] (world axis a): normalisation and to_local folded in
    float deta[3];                         // d eta / d s[a]
};
static_assert(sizeof(SeqGradFrame<3>) == 4 * (2 * 32 + 12) && sizeof(SeqGradFrame<kNbWavelengths>) == 4 * (2 * 112 + 12),
              "SeqGradFrame layout");
static_assert(offsetof(SeqGradFrame<3>, dsky_eta) == 128 && offsetof(SeqGradFrame<3>, dlocal) == 256 &&
              offsetof(SeqGradFrame<3>, deta) == 292 && offsetof(SeqGradFrame<kNbWavelengths>, dsky_eta) == 448 &&
              offsetof(SeqGradFrame<kNbWavelengths>, dlocal) == 896 && offsetof(SeqGradFrame<kNbWavelengths>, deta) == 932,
              "SeqGradFrame layout");
static_assert(sizeof(SeqGradFrame<3>) % 16 == 0 && sizeof(SeqGradFrame<kNbWavelengths>) % 16 == 0, "SeqGradFrame alignment");
constexpr size_t seq_grad_bytes(int nch) { return 4 * (size_t)(2 * seq_grad_block(nch) + 12); }

// sunsky_stage_sequence_grad: one workgroup per frame.  stages[k]: frame k's TangentStage
// scalars with every tangent 0 (tangent_stage_for); the kernel derives the turbidity tangent
// (dT = 1) and the unit-elevation tangent (dx = dx_per_eta) from it.
struct SeqGradStageArgs {
    void* grads;                   // SeqGradFrame<nch>[count], dlocal / deta filled
    const TangentStage* stages;    // [count], device
    const float* sky_params_ds;    // the sequence's own device copy of the sky datasets
    const float* sky_rad_ds;
    int nch, count;
};
static_assert(sizeof(SeqGradStageArgs) == 40, "SeqGradStageArgs layout");

// The reverse-mode kernels' launch shape.  Each wave keeps one row of 5 sums per frame
// (weight, turbidity, sun x / y / z): in LDS while count <= kSeqGradLdsFrames (4 waves x count
// x 5 floats of dynamic LDS, 40 KiB at the limit), added into one row per workgroup at the end;
// otherwise directly in the workspace, one row per wave.  The workspace is rows x count x 5
// floats; the grid is capped so that it stays within kSeqGradWorkspaceFloats (and never below
// one workgroup: 4 rows, 20 x count floats, once count > kSeqGradLdsFrames).
constexpr int kSeqGradSums = 5;
constexpr int kSeqGradLdsFrames = 512;
constexpr size_t kSeqGradWorkspaceFloats = (size_t)1 << 22;   // 16 MiB
constexpr int kSeqGradBlocksPerCu = 16;
constexpr int kSeqGradReduceBlock = 64;

// sunsky_sequence_eval_vjp_*: the gradient records, the cotangent and the workspace
struct SeqGradArgs {
    const void* grads;             // SeqGradFrame<nch>[count]
    const float* dout;             // cotangent planes
    size_t dstride;
    float* rows;                   // workspace [gridDim.x (LDS rows) or gridDim.x * 4][count][5]
    int lds_rows;                  // 1: the waves' rows live in dynamic LDS until the end
    int pad;
};
static_assert(sizeof(SeqGradArgs) == 40, "SeqGradArgs layout");

// ---------------------------------------------------------------- sequence sampling
// The sampling distribution of a sequence (sunsky_sequence_prepare_sampling), all in the
// emitter's local frame: one equal-solid-angle table of the cumulative sky's luminance
// (row i: z = cos theta in [i / nz, (i + 1) / nz), column j: phi in [j dphi, (j + 1) dphi))
// and one cone per frame.
//   pdf(d) = sky_coef f[cell(d)] + sun_coef sum_k q_k [dot(s_k, d) >= cos_cutoff]
// with sky_coef = w_sky / (S omega) and sun_coef = (1 - w_sky) sun_pdf.  Every CDF is
// normalised and inclusive (last entry 1); entry j is picked by u when cdf[j - 1] <= u < cdf[j].
constexpr size_t kSeqFrameQ = 10;   // SeqFrame::pad[0] as a float index: q_k, beside the header's scalar load
constexpr int kSeqSampleMaxZ = 1024, kSeqSampleMaxPhi = 4096, kSeqSampleMaxCells = 1 << 20;

struct SeqSampling {
    const float* f;            // [nz][nphi] cell values
    const float* row_cdf;      // [nz] marginal over the row sums
    const float* cell_cdf;     // [nz][nphi] per-row distribution
    const float* frame_cdf;    // [count] over q
    const float* suns;         // [count] x {s_k.xyz, q_k}: the pdf kernel's 16-byte records
    int nz, nphi;
    float w_sky, sky_coef, sun_coef;
    float dphi, inv_dphi;
    int pad;
};
static_assert(sizeof(SeqSampling) == 72 && offsetof(SeqSampling, nz) == 40, "SeqSampling layout");

// The sample kernels' batch: u, it.p (optional) and the mask in; ds.d, ds.pdf, ds.dist /
// ds.p (optional) and the weight planes out
struct SeqSampleIO {
    const float *ux, *uy, *px, *py, *pz;
    const uint8_t* active;
    float *dx, *dy, *dz, *pdf, *dist, *opx, *opy, *opz, *weight;
    size_t wstride;
};
static_assert(sizeof(SeqSampleIO) == 128, "SeqSampleIO layout");

// sunsky_sequence_table / sunsky_sequence_suns (prepare_sampling): one lane per cell / frame
struct SeqTableArgs {
    float* f;                  // [nz][nphi], written
    float* B;                  // [count] disc-centre luminance per frame, written
    float cie_y[kNbWavelengths];
    int nz, nphi;
    int pad;
};
static_assert(sizeof(SeqTableArgs) == 16 + 4 * kNbWavelengths + 12, "SeqTableArgs layout");

// ---------------------------------------------------------------- sequence irradiance
// sunsky_sequence_prepare_irradiance / sunsky_sequence_irradiance (sunsky_amd.h has the
// definition).  The sun flux F_k is a 4 x 16 rule over frame k's cone: 4 Gauss-Legendre nodes
// in u = cos psi on [0, 1] (kSeqFluxU, kSeqFluxG), 16 midpoints in azimuth; one lane per point.
constexpr int kSeqFluxNu = 4, kSeqFluxNphi = 16;
static_assert(kSeqFluxNu * kSeqFluxNphi == 64, "one wave per frame, one lane per point of the rule");
constexpr double kSeqFluxU[kSeqFluxNu] = {0.06943184420297371, 0.33000947820757187, 0.66999052179242813,
                                          0.93056815579702629};
constexpr double kSeqFluxG[kSeqFluxNu] = {0.17392742256872693, 0.32607257743127307, 0.32607257743127307,
                                          0.17392742256872693};
constexpr int kSeqIrrMaxPlanes = kMaxBroadcastLambda;
constexpr size_t kSeqIrrMaxValues = (size_t)1 << 22;   // n_z n_phi n_planes

// Floats of one record of the staged image: a direction (cell centre c_ij or sun s_k), then the
// n_planes weighted values (omega R_p[i, j] or w_k F_k[p]), padded to 16 bytes.  8 for RGB.
constexpr int seq_irr_record(int planes) { return (3 + planes + 3) & ~3; }
static_assert(seq_irr_record(3) == 8 && seq_irr_record(1) == 4 && seq_irr_record(kSeqIrrMaxPlanes) == 36, "record size");

// Point (a, b) of the flux rule for a cone of sin^2(half aperture) = s2: the direction in the
// sun's frame (sin gamma cos phi, sin gamma sin phi, cos gamma) and the ring weight
// W_a = g_a u_a s2 / cos gamma_a (sum_a W_a 2 pi = the cone's solid angle).
struct SeqFluxPoint { float x, y, z, u, W; };
SS_HD inline SeqFluxPoint seq_flux_point(float s2, int a, int b) {
    SS_NO_CONTRACT
    SeqFluxPoint p;
    p.u = (float)kSeqFluxU[a];
    const float sin2 = (1.f - p.u * p.u) * s2;
    p.z = sqrtf(1.f - sin2);
    const float sg = sqrtf(sin2);
    const float phi = ((float)b + 0.5f) * (kTwoPi / (float)kSeqFluxNphi);
    p.x = sg * cosf(phi);
    p.y = sg * sinf(phi);
    p.W = (float)kSeqFluxG[a] * p.u * s2 / p.z;
    return p;
}

// sunsky_sequence_irradiance_table / sunsky_sequence_irradiance_flux (prepare_irradiance): one
// lane per cell, one wave per frame.  L: the spectral wavelength list (m = n_planes), unused for RGB.
struct SeqIrrTableArgs {
    float* sky;                // [planes][nz][nphi] R_p, written
    float* flux;               // [planes][count] F_k[p], written
    LambdaSet L;
    int nz, nphi, planes;
    float sin2_half_ap;        // sin^2(half aperture) = 1 / SunskyKArgs::inv_sin2_half_ap
};
static_assert(sizeof(SeqIrrTableArgs) == 16 + sizeof(LambdaSet) + 4 + 16 && offsetof(SeqIrrTableArgs, nz) == 16 + sizeof(LambdaSet),
              "SeqIrrTableArgs layout");

// The hot path's view: the staged image.  Every record is 16-byte aligned and read with one
// address per wave.
struct SeqIrradiance {
    const float* cells;        // [ncells] records: c_ij.xyz, omega R_p[i, j]
    const float* suns;         // [nsuns] records: s_k.xyz, w_k F_k[p] (frames with a zero flux left out, order kept)
    int nz, nphi, nsuns, planes;
};
static_assert(sizeof(SeqIrradiance) == 32 && offsetof(SeqIrradiance, nz) == 16, "SeqIrradiance layout");

// sunsky_sequence_irradiance_horizon: the horizon profiles beside the image.  Sector b's plane
// starts at h + b * stride; receiver r reads element r * per_receiver of it (0: one shared profile).
struct SeqIrrHorizon {
    const float* h;            // [sectors] planes of sin(horizon elevation)
    const int* sun_cols;       // [nsuns] column j_k of the image's suns, in the image's order
    size_t stride;             // floats between two sectors' planes
    int sectors, sector_len;   // sector_len = nphi / sectors columns each
    int per_receiver;          // 1: element r of a plane is receiver r's; 0: element 0 is everyone's
    int pad;
};
static_assert(sizeof(SeqIrrHorizon) == 40 && offsetof(SeqIrrHorizon, sectors) == 24, "SeqIrrHorizon layout");

// ---------------------------------------------------------------- per-frame irradiance series
// sunsky_sequence_prepare_irradiance_series / sunsky_sequence_irradiance_series (sunsky_amd.h has
// the definition).  The frames are staged in groups of G consecutive frames, G a function of the
// plane count P alone: as many frames as fit kSeqIrrSeriesWidth values, at most
// kSeqIrrSeriesMaxGroup, at least one (RGB: 8 frames, 24 values).  A group's image is the
// forward's image with G * P "planes": per cell one record c_ij.xyz, then value g * P + p =
// A^{kG+g}_p[i, j], padded to 16 bytes (seq_irr_record(G * P)); a frame past the last one holds
// zeros.  Beside the images lie one 16-byte sun record {s_k.xyz, F_k[p]} and one sun column j_k
// per value.  A work item of the hot path is (receiver pair, group); value v of group gr is
// output plane gr * G * P + v - first_frame * P, stored when it falls into the call's range.
constexpr int kSeqIrrSeriesWidth = 24;       // values per group: the widest pass of the contraction
constexpr int kSeqIrrSeriesMaxGroup = 8;     // frames per group at most
constexpr size_t kSeqIrrSeriesMaxFloats = (size_t)1 << 26;   // the cap of K * P * n_z * n_phi
constexpr int seq_irr_series_group(int planes) {
    return kSeqIrrSeriesWidth / planes < 1 ? 1
           : kSeqIrrSeriesWidth / planes > kSeqIrrSeriesMaxGroup ? kSeqIrrSeriesMaxGroup : kSeqIrrSeriesWidth / planes;
}
static_assert(seq_irr_series_group(3) == 8 && seq_irr_series_group(1) == 8 && seq_irr_series_group(5) == 4 &&
              seq_irr_series_group(kSeqIrrMaxPlanes) == 1, "group size");

// sunsky_sequence_irradiance_series_table: one lane per (cell, group).  Writes the groups' images
// (image != nullptr: `groups` groups of `group` frames from frame `frame0`, records of `rec`
// floats, value = omega * sky, direction = the forward image's, which the host computed) or one frame's plain table (raw != nullptr: [planes][nz][nphi] of
// frame `frame0`, group = groups = 1, value = sky).
struct SeqIrrSeriesTableArgs {
    float* image;
    float* raw;
    const float* cells;        // the forward's image: a record's direction is copied from its cell record
    LambdaSet L;
    int nz, nphi, planes;
    int group, groups, rec, frame0;
    float omega;
    int cells_rec;             // floats of one record of the forward's image
};
static_assert(offsetof(SeqIrrSeriesTableArgs, nz) == 24 + sizeof(LambdaSet) &&
              sizeof(SeqIrrSeriesTableArgs) == 24 + sizeof(LambdaSet) + 36, "SeqIrrSeriesTableArgs layout");

// The hot path's view of the staged series and of one call's range of frames
struct SeqIrrSeries {
    const float* images;       // [groups] images of nz * nphi records of `rec` floats
    const float* suns;         // [groups][values] records {s_k.xyz, F_k[p]}
    const int* sun_cols;       // [groups][values] column j_k of the value's frame
    size_t image_floats;       // floats of one group's image: nz * nphi * rec
    long long plane0;          // first_frame * planes: value v of group gr is plane gr * values + v - plane0
    long long n_planes;        // n_frames * planes: the planes the call stores
    int nz, nphi;
    int values, rec;           // G * P, and seq_irr_record(values)
    int group0, n_groups;      // the groups the call's frames lie in
};
static_assert(sizeof(SeqIrrSeries) == 72 && offsetof(SeqIrrSeries, nz) == 48, "SeqIrrSeries layout");

// ---------------------------------------------------------------- gradients of the sequence irradiance
// sunsky_sequence_prepare_irradiance_grad / sunsky_sequence_irradiance_vjp (sunsky_amd.h has the
// definition).  The weight gradient goes through the adjoint image: per slice of receivers one
// workspace row [planes][cells + count] (G_p over the cells, then H_p over every frame's sun),
// written by sunsky_sequence_irradiance_adjoint; sunsky_sequence_irradiance_grad_fold adds the
// rows in slice order and contracts the sum with each frame's sky and flux.
constexpr int kSeqIrrGradChunk = 256;          // receivers per chunk sum: one per lane of the workgroup that stages them
constexpr int kSeqIrrGradCellsPerLane = 4;     // entries (cells or suns) a lane of the adjoint kernel owns
constexpr int kSeqIrrGradTile = kSeqIrrGradChunk * kSeqIrrGradCellsPerLane;   // entries per workgroup
constexpr int kSeqIrrGradSpecPlanes = 4;       // planes per pass of the adjoint kernel (spectral; RGB: 3, one pass)
constexpr size_t kSeqIrrGradSliceMin = 1024;   // receivers: no slice is cut shorter
constexpr unsigned kSeqIrrGradMaxSlices = 64;
constexpr size_t kSeqIrrGradWorkspaceFloats = (size_t)1 << 22;   // 16 MiB: the cap of slices x planes x (cells + count)
constexpr int kSeqIrrGradAdjointBlocksPerCu = 8, kSeqIrrGradFoldBlocksPerCu = 8;

// The slices of n receivers: their number and length, a function of (n, planes, cells, count)
// and the workspace bound only.  slices = ceil(n / kSeqIrrGradSliceMin) capped by
// kSeqIrrGradMaxSlices and by the rows the bound holds (never below 1); the length is
// ceil(n / slices) rounded up to whole chunks, and the slices in use are ceil(n / length).
struct SeqIrrGradShape {
    unsigned slices, slice_len;
};
inline unsigned seq_irr_grad_max_slices(int planes, size_t cells, int count, size_t cap_floats) {
    const size_t row = (size_t)planes * (cells + (size_t)count), fit = cap_floats / row;
    return (unsigned)(fit < 1 ? 1 : fit < kSeqIrrGradMaxSlices ? fit : kSeqIrrGradMaxSlices);
}
inline SeqIrrGradShape seq_irr_grad_shape(size_t n, int planes, size_t cells, int count, size_t cap_floats) {
    const size_t most = seq_irr_grad_max_slices(planes, cells, count, cap_floats);
    size_t want = (n + kSeqIrrGradSliceMin - 1) / kSeqIrrGradSliceMin;
    want = want < 1 ? 1 : want < most ? want : most;
    size_t len = (n + want - 1) / want;
    len = (len + kSeqIrrGradChunk - 1) / kSeqIrrGradChunk * kSeqIrrGradChunk;
    if (len < (size_t)kSeqIrrGradChunk) len = kSeqIrrGradChunk;
    return SeqIrrGradShape{(unsigned)((n + len - 1) / len), (unsigned)len};
}

// What the three gradient kernels read beside the forward's image
struct SeqIrrGrad {
    const float* suns;         // [count] x {s_k.xyz, 0}: every frame's local sun direction
    const float* flux;         // [planes][count] F_k[p], unweighted
    float* rows;               // workspace [slices][planes][cells + count]
    const float* dout;         // cotangent planes
    size_t dstride;
    float omega;
    int count;
    unsigned slices, slice_len;
};
static_assert(sizeof(SeqIrrGrad) == 56 && offsetof(SeqIrrGrad, omega) == 40, "SeqIrrGrad layout");

// ---------------------------------------------------------------- ... under a horizon profile
// sunsky_sequence_irradiance_horizon_vjp (sunsky_amd.h has the definition).  The kernels take the
// forward's SeqIrrHorizon beside SeqIrrGrad; the adjoint's sun_cols are the columns of all K
// frames, which prepare_irradiance_grad stages behind the fluxes.  The adjoint's work units are
// sector-aware: per sector ceil(n_z sector_len / tile) tiles of its cells, then ceil(K / tile)
// tiles of the suns; a tile has 256 lanes x 2 entries where a sector has at most
// kSeqIrrHzGradNarrowCells cells, 256 x 4 otherwise.  The workspace row layout, the slices and
// the fold are sunsky_sequence_irradiance_vjp's.
constexpr int kSeqIrrHzGradNarrowCells = 512;
inline size_t seq_irr_hz_grad_units(int nz, int sector_len, int sectors, int count) {
    const size_t sector_cells = (size_t)nz * (size_t)sector_len;
    const size_t tile = (size_t)kSeqIrrGradChunk * (sector_cells > (size_t)kSeqIrrHzGradNarrowCells ? 4 : 2);
    return (size_t)sectors * ((sector_cells + tile - 1) / tile) + ((size_t)count + tile - 1) / tile;
}

}  // namespace sunsky
