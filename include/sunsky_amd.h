/*
 * sunsky_amd.h -- C ABI of the MI355X-native sun/sky emitter.
 *
 * Drop-in replacement for the `sunsky` emitter plugin of
 * matttsss/mitsuba3-sunsky (src/emitters/sunsky.cpp).  Each entry point names
 * the reference interface it replaces (file:line under the reference tree).
 * Conventions:
 *   - every function returns an int status (SUNSKY_OK = 0); on failure the
 *     thread-local message from sunsky_last_error() carries the reference's
 *     error text (the reference throws through Log(Error, ...), logger.cpp:55-60);
 *     nothing throws across this boundary;
 *   - batch inputs/outputs are DEVICE pointers (HBM), structure-of-arrays,
 *     one fp32 plane per component -- the layout Dr.Jit gives the JIT variants;
 *     multi-channel outputs are planes at `out + c * out_stride`;
 *   - `active` is an optional per-ray uint8 mask (NULL = all active), the
 *     `Mask active` argument of the reference methods;
 *   - `stream` is a hipStream_t (NULL = default stream); every batch call is
 *     asynchronous and stream-ordered.  The hot-path calls (eval,
 *     eval_direction, eval_spectral_broadcast, sample_direction, pdf_direction,
 *     sample_ray, sample_wavelengths, direct_diffuse, direct_diffuse_rays,
 *     eval_jvp_dir, eval_vjp_dir, sequence_eval, sequence_sample_direction,
 *     sequence_pdf_direction, sequence_eval_vjp, sequence_irradiance,
 *     sequence_irradiance_horizon, sequence_irradiance_vjp,
 *     sequence_irradiance_horizon_vjp, sequence_irradiance_series)
 *     allocate nothing, make no host-synchronous call and may be captured into
 *     a hipGraph (tests/test_graph_capture.py).  Kernels read the emitter state
 *     from device memory, which parameters_changed_async rewrites in place on
 *     the caller's stream, so a captured graph replays with the state current at
 *     replay.  eval_jvp and eval_vjp restage their tangent tables (host fp64
 *     derivative of the staging, stream-ordered copy from pinned memory) when
 *     the emitter state (or, for eval_jvp, the tangent) changed since the
 *     previous call; they and bake_latlong order successive calls on the same
 *     emitter through events and are not capturable;
 *   - every batch entry point opens a roctx range "<ProfilerPhase>:<entry>"
 *     (the reference's MI_MASKED_FUNCTION scopes; SUNSKY_AMD_ROCTX=0 disables);
 *   - create/update/destroy are host-synchronous and must not race batch calls
 *     on the same emitter (the reference's parameters_changed() contract).
 */
#ifndef SUNSKY_AMD_H
#define SUNSKY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUNSKY_AMD_ABI_VERSION 7   /* 3: direct_diffuse visibility, direct_diffuse_rays; 4: direct_conductor(_rays),
                                     emitter_tangent_tables, direct_diffuse draws sample_1 (path.cpp:233);
                                     5: direct_conductor(_rays)_aniso (alpha_u, alpha_v);
                                     6: SUNSKY_TABLE_SUN_SKY_FIT, emitter_inject_staging_fault (testing),
                                        a rejected update reverts to the last accepted one;
                                     7: SUNSKY_TABLE_SUN_SEGMENTS, emitter_sun_segments (testing);
                                        added since, additive only (the version stays 7):
                                        eval_jvp_dir, eval_vjp_dir; sun_coordinates and the
                                        sunsky_sequence_* calls (frame sequences, their
                                        sampling, update, gradients, irradiance, the
                                        irradiance's gradients, the irradiance under a
                                        horizon profile and the per-frame irradiance
                                        series included) */

typedef enum sunsky_status {
    SUNSKY_OK = 0,
    SUNSKY_ERROR_INVALID_VALUE = 1,   /* bad parameter (reference: Log(Error, ...))      */
    SUNSKY_ERROR_FILE = 2,            /* dataset missing / unreadable (sunsky.h:519-520) */
    SUNSKY_ERROR_FORMAT = 3,          /* dataset header / size mismatch (sunsky.h:531)   */
    SUNSKY_ERROR_HIP = 4,             /* HIP runtime / code object failure               */
    SUNSKY_ERROR_NOT_IMPLEMENTED = 5, /* sample_position (sunsky.cpp:483-495)            */
    SUNSKY_ERROR_INTERNAL = 6,
    SUNSKY_ERROR_COMM = 7             /* RCCL unavailable / communicator failure         */
} sunsky_status;

typedef enum sunsky_variant {     /* mitsuba.conf variants: *_rgb / *_spectral */
    SUNSKY_VARIANT_RGB = 0,
    SUNSKY_VARIANT_SPECTRAL = 1
} sunsky_variant;

typedef enum sunsky_semantics {
    SUNSKY_SEMANTICS_JIT = 0,     /* llvm_* / cuda_*: quadrature sky/sun ratio (sunsky.cpp:784-885) */
    SUNSKY_SEMANTICS_SCALAR = 1   /* scalar_*: ratio 0.5, uniform wavelength pdf (:778-783)         */
} sunsky_semantics;

typedef enum sunsky_precision {
    SUNSKY_PRECISION_FAST = 0,      /* host-folded transcendental constants (default) */
    SUNSKY_PRECISION_REFERENCE = 1  /* reference operation order, full-precision libm */
} sunsky_precision;

typedef enum sunsky_table_id {      /* staged tables, for inspection / parity tests */
    SUNSKY_TABLE_SKY_PARAMS = 0,    /* nch x 9  (m_sky_params)            */
    SUNSKY_TABLE_SKY_RADIANCE = 1,  /* nch      (m_sky_radiance)          */
    SUNSKY_TABLE_SUN_RADIANCE = 2,  /* 45x3x4x6 or 45x11x4 (m_sun_radiance) */
    SUNSKY_TABLE_SUN_LD = 3,        /* 11 x 6   (m_sun_ld)                 */
    SUNSKY_TABLE_GAUSSIANS = 4,     /* 20 x 5   (m_gaussians)              */
    SUNSKY_TABLE_GAUSSIAN_CDF = 5,  /* 20       (DiscreteDistribution cdf) */
    SUNSKY_TABLE_SPECTRAL_PDF = 6,  /* m_spectral_distr pdf                */
    SUNSKY_TABLE_SPECTRAL_CDF = 7,  /* m_spectral_distr cdf                */
    SUNSKY_TABLE_ALBEDO = 8,        /* extract_albedo() result             */
    SUNSKY_TABLE_SUN_SKY_FIT = 9,   /* 10: the FAST samplers' sun-pick sky pdf fit: c0..c5, bound,
                                       smallest value, usable (0/1), in use for this w_sky (0/1) */
    SUNSKY_TABLE_SUN_SEGMENTS = 10  /* 47: render_sun's segment decision (sunsky.cpp:579-584) as cos theta
                                       thresholds z[0..44] (z[j] = smallest fp32 cos theta whose segment
                                       is >= j), then the disc's first and last segment */
} sunsky_table_id;

#define SUNSKY_FLAG_INFINITE 0x04u          /* EmitterFlags::Infinite (emitter.h:29-30) */
#define SUNSKY_FLAG_SPATIALLY_VARYING 0x10u /* EmitterFlags::SpatiallyVarying (emitter.h:39-40) */

typedef struct sunsky_props sunsky_props;
typedef struct sunsky_emitter sunsky_emitter;

typedef struct sunsky_vec3_in { const float *x, *y, *z; } sunsky_vec3_in;
typedef struct sunsky_vec3_out { float *x, *y, *z; } sunsky_vec3_out;

typedef struct sunsky_info {
    int variant, semantics, nb_channels, active_record;
    float turbidity, sky_scale, sun_scale;
    float sun_half_aperture, cos_cutoff, area_ratio;
    float sun_dir_world[3];       /* m_sun_dir                 */
    float sun_dir_local[3];       /* m_local_sun_frame.n       */
    float sun_angles[2];          /* m_sun_angles (phi, theta) */
    float sky_sampling_w;         /* m_sky_sampling_w          */
    float bsphere_center[3], bsphere_radius;
    unsigned flags;               /* SUNSKY_FLAG_*             */
    int device;                   /* HIP device owning the tables */
    int precision;                /* sunsky_precision          */
} sunsky_info;

/* ------------------------------------------------------------ library */
int sunsky_abi_version(void);
const char *sunsky_last_error(void);

/* --------------------------------------------------- property bag
 * mitsuba::Properties as consumed by init_from_props (sunsky.cpp:889-948):
 * "turbidity", "sky_scale", "sun_scale", "sun_aperture" (deg), "albedo"
 * (float / per-channel spectrum / irregular spectrum), "sun_direction" (vector)
 * XOR {"latitude","longitude","timezone","year","month","day","hour",
 * "minute","second"}, "to_world" (4x4 row-major).  Unqueried names are an
 * error at create time, like the XML/dict loader (src/core/xml.cpp:1085-1102). */
int sunsky_props_create(sunsky_props **out);
void sunsky_props_destroy(sunsky_props *p);
int sunsky_props_set_float(sunsky_props *p, const char *name, double value);
int sunsky_props_set_int(sunsky_props *p, const char *name, int64_t value);
int sunsky_props_set_vector3(sunsky_props *p, const char *name, float x, float y, float z);
int sunsky_props_set_transform(sunsky_props *p, const char *name, const float matrix_row_major[16]);
int sunsky_props_set_spectrum(sunsky_props *p, const char *name, const float *values, int count);
int sunsky_props_set_irregular_spectrum(sunsky_props *p, const char *name, const float *wavelengths,
                                        const float *values, int count);

/* ------------------------------------------------------------ emitter
 * SunskyEmitter(const Properties&) -- sunsky.cpp:162-218.  The emitter lives on the
 * CURRENT HIP device: its state (one SunskyKArgs block + tables) is allocated there,
 * the radiance tables and the JIT sampling quadrature are staged there by kernels,
 * and every later call on the emitter runs on that device whatever device is current.  dataset_path: NULL for the
 * bundled pack, a .pack file, or a directory holding the reference's
 * resources/sunsky/datasets/<table>.bin files (path_to_dataset, sunsky.h:124-141). */
int sunsky_emitter_create(const sunsky_props *props, int variant, int semantics,
                          const char *dataset_path, sunsky_emitter **out);
/* Same staging without a device: batch calls on it fail; for inspecting the
 * staged tables (get_info / get_table / to_string) on machines without a GPU. */
int sunsky_emitter_create_host(const sunsky_props *props, int variant, int semantics,
                               const char *dataset_path, sunsky_emitter **out);
void sunsky_emitter_destroy(sunsky_emitter *e);
/* traverse() parameters, sunsky.cpp:220-240 (name, 1/3/11/16 floats).  Values take
 * effect at the next parameters_changed; a rejected update (e.g. turbidity 12) restores
 * the last committed values. */
int sunsky_emitter_set_param(sunsky_emitter *e, const char *name, const float *values, int count);
/* Current value of a traverse() parameter: *count values written to out (<= capacity). */
int sunsky_emitter_get_param(const sunsky_emitter *e, const char *name, float *out, int capacity,
                             int *count);
/* parameters_changed(), sunsky.cpp:242-285, stream-ordered: validation and the cheap
 * geometry / TGMM staging run on the host; the radiance tables (sunsky.h:158-231,
 * 404-419) and the JIT quadrature (estimate_sky_sun_ratio, sunsky.cpp:772-886) run as
 * kernels on `stream`, writing the emitter's device state in place.  Batch calls on
 * `stream` after this one see the new state; the call does not wait for the device.
 * Work on other streams must be ordered by the caller (the reference's contract:
 * parameters_changed is not concurrent with rendering).  Not capturable: called on a
 * stream that is capturing a hipGraph it returns SUNSKY_ERROR_INVALID_VALUE and changes
 * nothing (update outside the capture; captured batch calls read the current state).
 * An update the device staging rejects (a negative wavelength-distribution node, as
 * ContinuousDistribution's constructor checks) is reported by the next call that reads
 * the state back (get_info / get_table / the blocking form), which restores and restages
 * the parameters of the last staging known to be accepted (every update queued since that
 * read-back is rolled back: the rejection status is sticky across stagings, so one
 * rejected update among several queued ones is never lost). */
int sunsky_emitter_parameters_changed_async(sunsky_emitter *e, void *stream);
/* TESTING ONLY (tests/test_graph_capture.py): the next `count` device stagings of `e`
 * report a rejected wavelength distribution, so the rollback path above can be exercised
 * without a parameter set that produces one.  0 turns it off. */
int sunsky_emitter_inject_staging_fault(sunsky_emitter *e, int count);
/* TESTING ONLY (tests/test_gpu_parity.py): pos[i] = the elevation segment render_sun
 * (sunsky.cpp:579-584) takes for a direction inside the sun disc whose cos theta is
 * cos_theta[i], decided by the code the emitter's eval and sampling kernels run (its
 * precision).  Device int32 output; defined for the cos theta of disc directions. */
int sunsky_emitter_sun_segments(const sunsky_emitter *e, const float *cos_theta, size_t n, int *pos, void *stream);
/* Blocking form: _async on the default (null) stream, then waits for the staging. */
int sunsky_emitter_parameters_changed(sunsky_emitter *e);
/* set_scene(), sunsky.cpp:287-301: bounding sphere of the scene bbox */
int sunsky_emitter_set_scene(sunsky_emitter *e, int bbox_valid, const float center[3], float radius);
int sunsky_emitter_set_precision(sunsky_emitter *e, int precision);
int sunsky_emitter_get_info(const sunsky_emitter *e, sunsky_info *out);
int sunsky_emitter_get_table(const sunsky_emitter *e, int table_id, float *out, size_t capacity,
                             size_t *count);
/* to_string(), sunsky.cpp:502-519 */
int sunsky_emitter_to_string(const sunsky_emitter *e, char *buf, size_t capacity);
/* bbox(), sunsky.cpp:498-500: always an invalid box (min=+inf, max=-inf) */
int sunsky_emitter_bbox(const sunsky_emitter *e, float out_min[3], float out_max[3]);

/* ------------------------------------------------------ batched hot path */
/* eval(si, active), sunsky.cpp:303-352.  wi = si.wi.
 * RGB: out = 3 planes.  Spectral: wavelengths = n_wavelengths planes (per-ray
 * si.wavelengths, Mitsuba uses 4) at `wavelengths + k * wl_stride`; out likewise. */
int sunsky_eval(const sunsky_emitter *e, sunsky_vec3_in wi, const float *wavelengths,
                int n_wavelengths, size_t wl_stride, const uint8_t *active, size_t n,
                float *out, size_t out_stride, void *stream);
/* eval_direction(it, ds, active), sunsky.cpp:453-461: eval with wi = -ds.d */
int sunsky_eval_direction(const sunsky_emitter *e, sunsky_vec3_in d, const float *wavelengths,
                          int n_wavelengths, size_t wl_stride, const uint8_t *active, size_t n,
                          float *out, size_t out_stride, void *stream);
/* Spectral eval of ONE host-side wavelength list broadcast to every ray (the
 * eval_full_spec layout of test_sunsky.py:42-59): out plane k = lambda[k]. */
int sunsky_eval_spectral_broadcast(const sunsky_emitter *e, sunsky_vec3_in wi,
                                   const float *wavelengths_host, int n_wavelengths,
                                   const uint8_t *active, size_t n, float *out,
                                   size_t out_stride, void *stream);
/* sample_direction(it, sample, active), sunsky.cpp:399-441.
 * it_p: interaction positions (x == NULL -> origin).  Outputs ds.d (required),
 * ds.pdf (required), ds.dist / ds.p (optional, NULL to skip); weight planes:
 * 3 (RGB) or n_wavelengths (spectral, wavelengths = it.wavelengths). */
int sunsky_sample_direction(const sunsky_emitter *e, const float *sample_x, const float *sample_y,
                            sunsky_vec3_in it_p, const float *wavelengths, int n_wavelengths,
                            size_t wl_stride, const uint8_t *active, size_t n, sunsky_vec3_out ds_d,
                            float *ds_pdf, float *ds_dist, sunsky_vec3_out ds_p, float *weight,
                            size_t weight_stride, void *stream);
/* pdf_direction(it, ds, active), sunsky.cpp:443-451 */
int sunsky_pdf_direction(const sunsky_emitter *e, sunsky_vec3_in ds_d, const uint8_t *active,
                         size_t n, float *pdf, void *stream);
/* sample_ray(time, wavelength_sample, sample2, sample3, active), sunsky.cpp:354-397.
 * Outputs ray.o, ray.d, ray.wavelengths (4 planes; zeros in RGB) and weight
 * (3 planes RGB / 4 spectral). */
int sunsky_sample_ray(const sunsky_emitter *e, const float *wavelength_sample, const float *sample2_x,
                      const float *sample2_y, const float *sample3_x, const float *sample3_y,
                      const uint8_t *active, size_t n, sunsky_vec3_out ray_o, sunsky_vec3_out ray_d,
                      float *ray_wavelengths, size_t wl_stride, float *weight, size_t weight_stride,
                      void *stream);
/* sample_wavelengths(si, sample, active), sunsky.cpp:463-480 (wi = si.wi).
 * Outputs 4 wavelength planes and 4 (spectral) / 3 (RGB) weight planes. */
int sunsky_sample_wavelengths(const sunsky_emitter *e, sunsky_vec3_in wi, const float *sample,
                              const uint8_t *active, size_t n, float *wavelengths, size_t wl_stride,
                              float *weight, size_t weight_stride, void *stream);
/* sample_position(), sunsky.cpp:483-495: NotImplementedError in the reference */
int sunsky_sample_position(const sunsky_emitter *e);

/* Lat-long bake of the sky (a caller of eval, as sunsky-testing/sky_data_test.py:58-79
 * builds an environment map from eval over helpers.py get_spherical_rays): pixel (x, y)
 * of a width x height image holds eval(si.wi = -sphdir(theta_y, phi_x)) with
 * theta_y = linspace(theta0, theta1, height)[y], phi_x = linspace(phi0, phi1, width)[x]
 * (z-up, local frame of to_world applied).  Planes [c][height * width], row-major:
 * 3 RGB planes, or one per host wavelength (spectral).  Directions are generated on the
 * device: the bake only writes HBM. */
int sunsky_bake_latlong(const sunsky_emitter *e, int width, int height, float theta0, float theta1,
                        float phi0, float phi1, const float *wavelengths_host, int n_wavelengths,
                        float *out, size_t out_stride, void *stream);

/* ------------------------------------------------------------ frame sequences
 * A sequence is count >= 1 frames over a snapshot of one emitter: frame k has a world-space
 * sun direction s_k, a turbidity T_k in [1, 10] and a weight w_k (finite, >= 0); variant,
 * semantics, albedo, sky_scale, sun_scale, sun aperture, to_world and precision are the
 * emitter's at creation.  One call returns, per ray and output plane,
 *     out = sum_k w_k eval_k(wi)
 * where eval_k is sunsky_eval of an emitter that equals the parent with sun_direction = s_k
 * and turbidity = T_k: the same masks (horizon, per-frame sun-disc test), the same per-frame
 * elevation segment, and in FAST precision the same fp64 disc term.  Frames are added in
 * frame order in fp32 (fma(w_k, eval_k, acc)): the result is deterministic.  A frame whose sun
 * is below the horizon behaves as that emitter does (sky coefficients 0; not an error).
 * Inactive lanes (mask, or cos theta < 0) give exact zeros.  The sequence keeps no pointer to
 * the emitter: later updates of the emitter do not reach it and it may outlive the emitter.
 * A time-lapse, a cumulative-sky map or a time-averaged sky is one launch instead of one
 * restaging and one pass over the rays per instant.
 * Out of scope: per-ray wavelengths (their channel index is per lane, so a frame's record
 * would no longer be wave-uniform), per-ray frame indices, forward-mode AD over a sequence
 * (the reverse mode is sunsky_sequence_eval_vjp below), per-frame albedo / scales / aperture. */
typedef struct sunsky_sequence sunsky_sequence;
typedef struct sunsky_sequence_desc {
    int count;        /* frames                       */
    int variant;      /* sunsky_variant               */
    int nb_channels;  /* 3 (RGB) / 11 (spectral)      */
    int precision;    /* sunsky_precision             */
    int device;       /* HIP device; -1: host-only    */
} sunsky_sequence_desc;
/* compute_sun_coordinates (sunsky.h:284-374), fp32 as the emitter's time/location mode
 * evaluates it: the unit sun direction in the emitter's local frame (z up) for a date, a
 * time and a place -- what turns a list of times into frame directions (to_world applied by
 * the caller gives the world-space direction sunsky_sequence_create takes). */
int sunsky_sun_coordinates(int year, int month, int day, float hour, float minute, float second,
                           float latitude, float longitude, float timezone, float out[3]);
/* Host-synchronous, like sunsky_emitter_create; on the emitter's device.  sun_dirs: count x 3
 * host floats (normalised as the emitter's constructor does, sunsky.cpp:923); turbidity: count
 * host floats, NULL = the emitter's; weights: count host floats, NULL = 1.  Errors
 * (SUNSKY_ERROR_INVALID_VALUE): "Turbidity value %f is out of range [1, 10]" (sunsky.cpp:248),
 * a zero or non-finite direction, a negative or non-finite weight, count < 1.  The frames'
 * sky channels are staged by one kernel (one workgroup per frame) with the arithmetic of the
 * emitter's own staging: frame k's channels are bit for bit those of a single emitter with
 * that frame's parameters.  Over a host-only emitter (sunsky_emitter_create_host) the staging
 * runs on the host and batch calls on the sequence fail, as they do on the emitter. */
int sunsky_sequence_create(const sunsky_emitter *e, int count, const float *sun_dirs,
                           const float *turbidity, const float *weights, sunsky_sequence **out);
void sunsky_sequence_destroy(sunsky_sequence *seq);
int sunsky_sequence_info(const sunsky_sequence *seq, sunsky_sequence_desc *out);
int sunsky_sequence_set_precision(sunsky_sequence *seq, int precision);
/* Frame k as staged, for inspection and tests (any output may be NULL): its local sun
 * direction, weight, turbidity, nb_channels x 9 sky coefficients (SUNSKY_TABLE_SKY_PARAMS
 * layout) and nb_channels sky radiances. */
int sunsky_sequence_get_frame(const sunsky_sequence *seq, int k, float sun_dir_local[3], float *weight,
                              float *turbidity, float *sky_params, float *sky_radiance);
/* The weighted sum of eval(si) over the frames (wi = si.wi).  RGB: wavelengths_host = NULL,
 * 3 planes.  Spectral: one host wavelength list broadcast to every ray, the
 * sunsky_eval_spectral_broadcast layout (<= 32 wavelengths; out plane k = lambda[k]; an
 * invalid wavelength gives 0).  A hot-path call. */
int sunsky_sequence_eval(const sunsky_sequence *seq, sunsky_vec3_in wi, const float *wavelengths_host,
                         int n_wavelengths, const uint8_t *active, size_t n, float *out,
                         size_t out_stride, void *stream);
/* sunsky_bake_latlong of the weighted sum: the same grid, planes and contract (successive
 * bakes of one sequence are ordered through an event; not capturable). */
int sunsky_sequence_bake_latlong(const sunsky_sequence *seq, int width, int height, float theta0,
                                 float theta1, float phi0, float phi1, const float *wavelengths_host,
                                 int n_wavelengths, float *out, size_t out_stride, void *stream);

/* Importance sampling of a sequence.  The distribution lives in the emitter's local frame
 * (to_world is applied on the way out, as in sunsky_sample_direction) and has two parts:
 *  - one table of the cumulative sky over n_z x n_phi cells of equal solid angle
 *    omega = 2 pi / (n_z n_phi): row i covers z = cos theta in [i / n_z, (i + 1) / n_z) (row 0
 *    at the horizon, z = 1 in the last row), column j covers phi = atan2(y, x) wrapped to
 *    [0, 2 pi) in [j dphi, (j + 1) dphi), dphi = 2 pi / n_phi.  The cell value is
 *    f_ij = Y(sum_k w_k sky_k(centre)) >= 0, the sky term only, Y the luminance
 *    (0.212671 R + 0.715160 G + 0.072169 B; spectral: sum_c cie_y[c] L_c / 11 over the 11
 *    nodes), always in reference precision.  S = sum f_ij, sky mass M = S omega.
 *  - one cone per frame: B_k = Y of frame k's disc term alone at the disc centre (0 for a
 *    sun below the horizon), sun mass P = Omega_c sum_k w_k B_k with
 *    Omega_c = 2 pi (1 - cos_cutoff), q_k = w_k B_k / sum_k w_k B_k (all 0 when the sum is 0).
 * With w_sky = M / (M + P), for a local direction d with z >= 0
 *     pdf(d) = w_sky f_cell(d) / (S omega)
 *            + (1 - w_sky) sun_pdf sum_k q_k [dot(s_k, d) >= cos_cutoff]
 * (the sum in frame order in fp32; 0 for z < 0 and for inactive lanes).  A sample u = (u1, u2)
 * with u1 < w_sky picks the row from the marginal over the row sums with u2 and the column
 * from that row's distribution with u1 / w_sky, each with sample reuse:
 * z = min((i + t2) / n_z, 1), phi = (j + t1) dphi.  Otherwise frame k comes from the q
 * distribution with (u1 - w_sky) / (1 - w_sky) and d = Frame(s_k).to_world(
 * square_to_uniform_cone(t1, u2)), its z clamped to 1 like the sky pick's.  A sample is active
 * when its local z >= 0 (sunsky.cpp:413).  ds.pdf is the pdf above at ds.d taken back to the local frame, so it
 * equals sunsky_sequence_pdf_direction(ds.d) bit for bit, and the weight is
 * sum_k w_k eval_k(-ds.d) / ds.pdf (0 where the lane is inactive or the quotient not finite).
 *
 * sunsky_sequence_prepare_sampling builds the tables (two launches and a read-back):
 * host-synchronous like sunsky_sequence_create, not capturable, not to be called while
 * launches on the sequence are in flight; a second call replaces the tables.
 * 1 <= n_z <= 1024, 4 <= n_phi <= 4096, n_z n_phi <= 2^20.  M + P == 0 (every frame dark or
 * of zero weight) is SUNSKY_ERROR_INVALID_VALUE.  Works on host-only sequences too (the
 * tables then come from the host's libm and agree with the device's to ~1e-5). */
typedef struct sunsky_sequence_sampling_desc {
    int n_z, n_phi;
    float w_sky;       /* M / (M + P)                */
    float sky_mass;    /* M = S omega                */
    float sun_mass;    /* P = Omega_c sum_k w_k B_k  */
} sunsky_sequence_sampling_desc;
typedef enum sunsky_sequence_table_id {
    SUNSKY_SEQUENCE_TABLE_SKY = 0,        /* f: n_z x n_phi                                    */
    SUNSKY_SEQUENCE_TABLE_ROW_CDF = 1,    /* n_z: inclusive, normalised (last entry 1)         */
    SUNSKY_SEQUENCE_TABLE_CELL_CDF = 2,   /* n_z x n_phi: per row, inclusive, normalised       */
    SUNSKY_SEQUENCE_TABLE_Q = 3,          /* count                                             */
    SUNSKY_SEQUENCE_TABLE_FRAME_CDF = 4,  /* count: inclusive, normalised                      */
    SUNSKY_SEQUENCE_TABLE_B = 5           /* count                                             */
} sunsky_sequence_table_id;
int sunsky_sequence_prepare_sampling(sunsky_sequence *seq, int n_z, int n_phi);
int sunsky_sequence_sampling_info(const sunsky_sequence *seq, sunsky_sequence_sampling_desc *out);
/* Writes min(count, capacity) floats (out may be NULL to query count). */
int sunsky_sequence_get_sampling_table(const sunsky_sequence *seq, int id, float *out, size_t capacity,
                                       size_t *count);
/* sunsky_sample_direction's layout: sample planes, optional it_p, optional mask; ds_d, ds_pdf
 * and n_planes weight planes (3 RGB; spectral: one host wavelength list of <= 32 entries as
 * sunsky_sequence_eval takes it); ds_dist / ds_p optional, formed from the snapshot's bounding
 * sphere as the emitter forms them.  Both calls are hot-path calls (stream-ordered, no
 * allocation, capturable); before prepare_sampling they fail with SUNSKY_ERROR_INVALID_VALUE. */
int sunsky_sequence_sample_direction(const sunsky_sequence *seq, const float *sample_x, const float *sample_y,
                                     sunsky_vec3_in it_p, const float *wavelengths_host, int n_wavelengths,
                                     const uint8_t *active, size_t n, sunsky_vec3_out ds_d, float *ds_pdf,
                                     float *ds_dist, sunsky_vec3_out ds_p, float *weight, size_t weight_stride,
                                     void *stream);
int sunsky_sequence_pdf_direction(const sunsky_sequence *seq, sunsky_vec3_in ds_d, const uint8_t *active,
                                  size_t n, float *pdf, void *stream);

/* Per-frame gradients of the weighted sum (reverse mode) and the in-place update of the
 * frames: what fitting the weights, turbidities or sun positions of a sequence needs.
 * With a cotangent d_out in the layout of sunsky_sequence_eval's out and
 *     L = sum_i sum_p d_out[p, i] sum_k w_k eval_k(wi_i)[p],
 * sunsky_sequence_eval_vjp accumulates (+=) into three device arrays, any of which may be NULL:
 *     grad_weight[k]        += dL/dw_k   = sum_i sum_p d_out eval_k
 *     grad_turbidity[k]     += dL/dT_k   = w_k sum_i sum_p d_out d eval_k / d T_k
 *     grad_sun_dir[3 k + a] += dL/ds_k[a] = w_k sum_i sum_p d_out d eval_k / d s_k[a]  (world axis a)
 * eval_k and its derivatives are those of the single emitter frame k stands for, with
 * sunsky_eval_vjp's conventions: reference-precision arithmetic whatever the sequence's
 * precision; the horizon mask, the disc test, the elevation segment and the wavelength validity
 * are not differentiated; floor(T) is constant with d t_rem / dT = 1 (at T = 10 the masked
 * upper row behaves as it does there); a sun below the horizon has zero sky tangents; the disc
 * term is included (T through the sun table's turbidity-lerp slope, taken from the raw dataset
 * on the spot; s through cos psi).  The sequence normalises s_k, so d / d s_k is the single
 * emitter's gradient at s_k / |s_k| taken through the normalisation,
 * (I - s^ s^T) / |s_k| applied before to_world's linear part: it has no component along s_k.
 * Inactive lanes (mask, cos theta < 0) and invalid wavelengths contribute exactly 0; a frame
 * with w_k = 0 gets exact zeros in grad_turbidity and grad_sun_dir.  Gradients of the albedo,
 * the scales and the aperture (the snapshot's, not a frame's) are out of scope.
 *
 * sunsky_sequence_update replaces the frames of an existing sequence (the same count; a NULL
 * array keeps the current values) with sunsky_sequence_create's validation and messages; a
 * refused update leaves the sequence untouched.  The records are restaged in place by the code
 * create runs: afterwards get_frame and eval are bit for bit those of a sequence created with
 * the new values (host-only sequences too).  Host-synchronous, not capturable, not to be called
 * while launches on the sequence are in flight.  It drops the sampling distribution
 * (sample_direction / pdf_direction fail as before prepare_sampling until it is called again)
 * and restages the gradient records if they were prepared.
 *
 * sunsky_sequence_prepare_grad (host-synchronous, like prepare_sampling; works on host-only
 * sequences, staging on the host) stages one gradient record per frame -- the tangents of the
 * frame's sky tables along T (bit for bit the dsky of sunsky_emitter_tangent_tables(turbidity,
 * [1]) of its single emitter) and along a unit sun elevation, and per world axis the tangent
 * of the local sun direction and of the elevation -- and allocates the reduction workspace.
 * Before it sunsky_sequence_eval_vjp fails with SUNSKY_ERROR_INVALID_VALUE.
 * sunsky_sequence_get_frame_tangent returns frame k's record (any output may be NULL):
 * nb_channels x 10 floats d{A..I, rad} each, dsun_local[3 a + r] and deta[a].
 *
 * sunsky_sequence_eval_vjp is a hot-path call: stream-ordered, no allocation, no
 * host-synchronous call, capturable.  Arguments as sunsky_sequence_eval's, and d_out must not
 * be NULL; n == 0 succeeds and writes nothing.  The reduction is deterministic (wave shuffles,
 * one row of 5 sums per frame and wave, rows added in a fixed order; no float atomics): two
 * runs give the same bits.  The workspace belongs to the sequence: calls on one sequence from
 * different streams are the caller's to order.  It is bounded: one row of count x 5 floats per
 * workgroup of the launch (count <= 512: the 4 waves' rows are added up in LDS first) or per
 * wave (count > 512), and the grid is at most 16 workgroups per CU (SUNSKY_AMD_BLOCKS_PER_CU
 * overrides it) and shrinks as count grows so that the rows take at most 16 MiB -- or one
 * workgroup's 80 x count bytes where that is more. */
int sunsky_sequence_update(sunsky_sequence *seq, const float *sun_dirs, const float *turbidity,
                           const float *weights);
int sunsky_sequence_prepare_grad(sunsky_sequence *seq);
int sunsky_sequence_get_frame_tangent(const sunsky_sequence *seq, int k, float *dsky_turbidity,
                                      float *dsky_elevation, float dsun_local[9], float deta[3]);
int sunsky_sequence_eval_vjp(const sunsky_sequence *seq, sunsky_vec3_in wi, const float *wavelengths_host,
                             int n_wavelengths, const uint8_t *active, size_t n, const float *d_out,
                             size_t out_stride, float *grad_weight, float *grad_turbidity,
                             float *grad_sun_dir, void *stream);

/* Irradiance of the cumulative sky on oriented receivers: per output plane p and world-space
 * receiver normal n,
 *     E_p(n) ~ integral over the upper hemisphere of (sum_k w_k eval_k(-w))_p max(0, n . w) dw,
 * defined as a fixed quadrature so that it is deterministic and testable to rounding.
 *
 * Sky part.  The equal-solid-angle grid of the sampling table above: n_z x n_phi cells,
 * omega = 2 pi / (n_z n_phi), centres c_ij (z = (i + 1/2) / n_z, phi = (j + 1/2) 2 pi / n_phi)
 * in the emitter's local frame.  R_p[i, j] = (sum_k w_k sky_k(c_ij))_p: the sky term only (the
 * disc branch off), always reference precision, the frames added in frame order as
 * fma(w_k, v, acc) -- what the sampling table computes before it takes the luminance.
 * Planes: 3 for RGB; spectral: one per entry of a host wavelength list given at prepare time
 * (<= 32), each the lerp of its two neighbouring nodes as sunsky_sequence_eval forms it, an
 * invalid wavelength a plane of zeros.
 *
 * Sun part.  One flux per frame and plane, F_k[p]: the integral of frame k's disc term alone
 * (what eval adds on top of the sky inside the disc) over its cone, by a 4 x 16 rule:
 * u_a, g_a the 4 Gauss-Legendre nodes and weights on [0, 1] in u = cos psi, s2 = sin^2(half
 * aperture), sin^2 gamma_a = (1 - u_a^2) s2, cos gamma_a = sqrt(1 - sin^2 gamma_a), ring
 * weight W_a = g_a u_a s2 / cos gamma_a (2 pi sum_a W_a = Omega_c up to the rule),
 * phi_b = (b + 1/2) 2 pi / 16, d_ab = Frame(s_k).to_world(sin gamma_a cos phi_b,
 * sin gamma_a sin phi_b, cos gamma_a) with the samplers' coordinate_system.  v_ab[p] is the
 * disc term with cos theta = min(d_ab.z, 1), the elevation segment eval takes for it, and
 * cos psi = u_a as given: it is not recomputed from the rounded fp32 direction and there is no
 * dot >= cos_cutoff test (the outermost node lies within 0.5 % of the cone's cos range of the
 * edge, less than one fp32 ulp of the dot product at the default aperture).  v_ab = 0 where
 * d_ab.z < 0; F_k = 0 when s_k.z < 0.  F_k[p] = (2 pi / 16) sum_ab W_a v_ab[p], the 64 terms
 * added by a fixed binary tree (term l += term l + off for off = 32, 16, .., 1).  The limb
 * darkening is a degree-5 polynomial in cos psi, so the radial integrand is a degree-6
 * polynomial in u and 4 nodes are exact for it apart from the slow variation of the elevation
 * across the disc: against the same rule at 48 x 256 in fp64, 3.6e-6 relative for discs wholly
 * above the horizon (at a 5 degree aperture).  A disc that straddles the horizon is only
 * roughly integrated (about 5 % for a 2 degree sun with a 5 degree aperture).  RGB fluxes can
 * be negative in one channel (a low sun's blue); they are not clamped.
 *
 * Receiver.  With n_l = to_local(n), used as given (not renormalised),
 *     E_p(n) = sum_i sum_j omega R_p[i, j] max(0, n_l . c_ij) + sum_k w_k F_k[p] max(0, n_l . s_k).
 * The sun is a directional source carrying the disc's flux, with the cosine taken at the disc
 * centre: for a disc wholly in front of the receiver that is off by at most 1 - cos_cutoff,
 * relative.  Only the upper local hemisphere contributes.  Out of scope: light reflected by the
 * ground, occlusion other than a horizon profile (sunsky_sequence_irradiance_horizon below; no
 * near-field or per-cell visibility masks), per-receiver wavelength lists, and the gradients of E
 * with respect to a frame's turbidity and sun direction (they need a tangent of the flux rule;
 * the gradients with respect to the normals and the weights are below).
 * Inactive lanes (mask) give exact zeros.
 *
 * Summation order (the contract; independent of n, of the grid and of the lane, so two runs and
 * any launch shape give the same bits; no float atomics).  The products omega R_p[i, j] and
 * w_k F_k[p] are rounded to fp32 once at prepare time.  Per plane: each row's cells in column
 * order into a row sum that starts at 0, fma(max(0, n_l . c_ij), omega R_p[i, j], row); the row
 * sums in row order (row 0 first) into the plane's sum; then the suns in frame order,
 * fma(max(0, n_l . s_k), w_k F_k[p], sum) (frames whose w_k F_k is 0 in every plane add
 * nothing).  Every dot product is fma(a.z, b.z, fma(a.y, b.y, a.x b.x)).  The sequential depth
 * is n_phi + n_z + count fp32 additions per plane.
 *
 * Measured discretisation of the sky part against a converged quadrature (768 x 1536
 * Gauss-Legendre x trapezoid, which agrees with 512 x 1024 to 3e-6), worst relative error over
 * six normals (horizontal, 35 degree tilt, three vertical, one facing 30 degrees down):
 *     8 x 16: 6e-2     16 x 32: 1.9e-2     64 x 256: 1.6e-3     128 x 512: 5e-4
 *
 * sunsky_sequence_prepare_irradiance builds the tables (two launches and a read-back) and stages
 * the image the hot path walks: host-synchronous, not capturable, not to be called while
 * launches on the sequence are in flight; a second call replaces the tables.  n_z and n_phi as
 * prepare_sampling's, and n_z n_phi n_planes <= 2^22.  wavelengths_host: NULL / 0 for RGB,
 * 1..32 entries for spectral.  Independent of prepare_sampling: either, both or neither may be
 * prepared.  Works on host-only sequences (the tables then come from the host's libm).
 * sunsky_sequence_update drops the tables, as it drops the sampling distribution.
 * get_irradiance_table: SKY is n_planes x n_z x n_phi values R_p[i, j] (not multiplied by
 * omega), SUN_FLUX is n_planes x count values F_k[p] (not multiplied by w_k).
 *
 * sunsky_sequence_irradiance is a hot-path call: stream-ordered, no allocation, no
 * host-synchronous call, capturable.  One receiver per lane; normal: three device planes;
 * out: n_planes planes at out + p * out_stride.  n == 0 succeeds; n < 2^32.  Before
 * prepare_irradiance it fails with SUNSKY_ERROR_INVALID_VALUE. */
typedef struct sunsky_sequence_irradiance_desc {
    int n_z, n_phi, n_planes;
    float omega;       /* 2 pi / (n_z n_phi) */
} sunsky_sequence_irradiance_desc;
typedef enum sunsky_sequence_irradiance_table_id {
    SUNSKY_SEQUENCE_IRRADIANCE_TABLE_SKY = 0,       /* R: n_planes x n_z x n_phi */
    SUNSKY_SEQUENCE_IRRADIANCE_TABLE_SUN_FLUX = 1   /* F: n_planes x count       */
} sunsky_sequence_irradiance_table_id;
int sunsky_sequence_prepare_irradiance(sunsky_sequence *seq, int n_z, int n_phi, const float *wavelengths_host,
                                       int n_wavelengths);
int sunsky_sequence_irradiance_info(const sunsky_sequence *seq, sunsky_sequence_irradiance_desc *out);
/* Writes min(count, capacity) floats (out may be NULL to query count). */
int sunsky_sequence_get_irradiance_table(const sunsky_sequence *seq, int id, float *out, size_t capacity,
                                         size_t *count);
int sunsky_sequence_irradiance(const sunsky_sequence *seq, sunsky_vec3_in normal, const uint8_t *active, size_t n,
                               float *out, size_t out_stride, void *stream);

/* The irradiance under a horizon profile: far shading, per azimuth sector the elevation below
 * which a receiver sees nothing (hills, the building across the street, the next row of panels).
 * Additive: sunsky_sequence_irradiance and its bits are untouched.
 *
 * A profile has H = n_sectors azimuth sectors in the emitter's local frame; H divides n_phi, and
 * sector b covers the columns [b n_phi / H, (b + 1) n_phi / H) of the prepared grid.  Its value
 * h[b] = sin(horizon elevation) is in z units and used as given in fp32.  Profiles come as H planes,
 * sector b's at horizon + b * horizon_stride: either one shared profile (n_profiles = 1: element 0
 * of each plane is every receiver's, the site's far horizon) or one per receiver (n_profiles = n:
 * element r of plane b is receiver r's).  With A_p = fp32(omega R_p) and B_k[p] = fp32(w_k F_k[p])
 * the staged image's values,
 *     v_r[i, b] = min(max(fma(-h_r[b], (float)n_z, (float)(i + 1)), 0), 1)
 *     E_p(n_r; h_r) = sum_i sum_j fp32(max(0, n_l . c_ij) v_r[i, b(j)]) A_p[i, j]
 *                   + sum_k [s_k.z >= h_r[b_k]] max(0, n_l . s_k) B_k[p].
 * v is the visible share of row i's cells in sector b: the grid has equal solid angle in z, so
 * the share of a cell above a horizon at height h is exactly linear in h.  The dot product and
 * the summation order are sunsky_sequence_irradiance's (a row's cells in column order into a row
 * sum from 0, the row sums in row order, then the image's suns in frame order, every
 * product-and-add one fma); the only addition is that the clamped cosine is multiplied by v and
 * rounded to fp32 before the fma.  The sun is a point source here: the test is the exact fp32
 * comparison s_k.z >= h (equality counts as visible), and a hidden sun adds nothing.  b_k is the
 * sector of sun k's column, b_k = j_k / (n_phi / H); j_k is staged at prepare_irradiance time on
 * the host: phi = atan2f(s_k.y, s_k.x), plus 2 pi when negative, then
 * j_k = min(max((int)(phi (float)n_phi / 2 pi), 0), n_phi - 1) -- the column the sampling table
 * takes for a direction; a sun at the pole has column 0.
 * sunsky_sequence_get_irradiance_sun_columns returns j_k for all count frames (those the image
 * leaves out included); it works on host-only sequences, and sunsky_sequence_update drops the
 * columns with the tables.
 *
 * Consequences.  h <= 0 in every sector gives sunsky_sequence_irradiance bit for bit (v = 1,
 * c 1 = c, and every sun of the image has z >= 0).  h > 1 in every sector gives exact zeros.  A NaN
 * in a profile is unspecified for that receiver only.  Inactive lanes give exact zeros.  The result
 * does not depend on n, on the grid or on the lane; a shared profile gives the bits of the same
 * profile repeated per receiver.
 *
 * Out of scope (the gradients are sunsky_sequence_irradiance_horizon_vjp's, below):
 * partial shading of a sun disc, near-field or per-cell visibility bitmaps, ground reflection,
 * and profiles whose H does not divide n_phi (the caller picks n_phi: 240 for 48 sectors).
 *
 * A hot-path call: stream-ordered, no allocation, no host-synchronous call, capturable.
 * n == 0 succeeds (nothing else is looked at); n < 2^32.  Refused with
 * SUNSKY_ERROR_INVALID_VALUE and a message, in this order: a NULL normal or out; a NULL horizon;
 * n >= 2^32; a sequence without prepare_irradiance; n_sectors < 1 or not a divisor of n_phi;
 * n_profiles other than 1 and n; horizon_stride < n with n_profiles == n and n_sectors > 1;
 * out_stride < n with more than one plane; a host-only sequence, as for the other launches. */
int sunsky_sequence_get_irradiance_sun_columns(const sunsky_sequence *seq, int *out, size_t capacity, size_t *count);
int sunsky_sequence_irradiance_horizon(const sunsky_sequence *seq, sunsky_vec3_in normal, const float *horizon,
                                       int n_sectors, size_t n_profiles, size_t horizon_stride,
                                       const uint8_t *active, size_t n, float *out, size_t out_stride, void *stream);

/* The per-frame irradiance series: what a receiver collects in each frame (an hourly power
 * profile, a day's illuminance curve, the hour a far wall starts to shade a window), K * P planes
 * in one call.  Additive: sunsky_sequence_irradiance(_horizon) and their bits are untouched.
 *
 * Notation as above: n_l = to_local(n) as given; c_ij and omega the prepared grid's cell centres
 * and solid angle; sky_{k,p}(c) frame k's term of R_p (reference precision, disc branch off;
 * spectral: the two-node lerp, an invalid wavelength a plane of zeros); F_k[p] the unweighted flux.
 *     A^k_p[i, j] = fp32(omega sky_{k,p}(c_ij))          rounded once at prepare time
 *     E^k_p(n)    = sum_i sum_j A^k_p[i, j] max(0, n_l . c_ij)  +  F_k[p] max(0, n_l . s_k)
 * and under a horizon profile, by the rule of sunsky_sequence_irradiance_horizon with the same
 * v_r[i, b], sectors, n_profiles in {1, n}, strides and sun column j_k,
 *     E^k_p(n_r; h_r) = sum_i sum_j fp32(max(0, n_l . c_ij) v_r[i, b(j)]) A^k_p[i, j]
 *                     + [s_k.z >= h_r[b_k]] max(0, n_l . s_k) F_k[p].
 * The weights do not enter: every frame counts, one with w_k = 0 included; the series is each
 * frame's own irradiance and the caller integrates.  A frame whose sun is below the horizon gives
 * exact zeros, and so do inactive lanes; a NaN in a profile is unspecified for that receiver only.
 *
 * Summation order, per frame and plane: sunsky_sequence_irradiance's for a sequence holding that
 * one frame -- each row's cells in column order into a row sum from 0 (fma(cos, A, row)), the row
 * sums in row order, then the frame's one sun (fma(cos_sun, F_k[p], sum)); the dot product is the
 * forward's, fma(a.z, b.z, fma(a.y, b.y, a.x b.x)); depth n_phi + n_z + 1.  The result does not
 * depend on n, the lane, the grid, SUNSKY_AMD_BLOCKS_PER_CU, on how frames are grouped in the
 * staged image or on the sub-range of frames a call asks for.
 * Consequence: take a one-frame sequence with frame k's direction and turbidity and weight 1,
 * prepared on the same grid and wavelength list.  Planes [k P, (k + 1) P) of the series are bit
 * for bit its sunsky_sequence_irradiance output, and under a horizon its
 * sunsky_sequence_irradiance_horizon output.
 * Out of scope: gradients of the series, weighted or cumulative-prefix variants, ground
 * reflection, per-cell visibility, partial shading of a disc.
 *
 * sunsky_sequence_prepare_irradiance_series is host-synchronous and needs prepare_irradiance.  It
 * is sticky exactly as prepare_irradiance_grad is (a later prepare_irradiance restages it,
 * sunsky_sequence_update drops it with the tables) and independent of it.  One kernel computes
 * A^k_p for all K frames on the device and writes the staged image there: the frames lie in
 * groups of G consecutive frames, G = min(8, max(1, 24 / P)) a function of P alone (8 for RGB),
 * a group's record being a cell direction followed by its G P values, 16-byte aligned; every
 * frame's s_k, F_k[p] and j_k lie beside them.  K P Q <= 2^26 floats (256 MiB), refused with a
 * message above that; the environment variable SUNSKY_AMD_IRRADIANCE_SERIES_MAX_FLOATS, read at
 * prepare time, lowers the cap (a restaging by prepare_irradiance whose tables exceed the cap
 * leaves the series unprepared).  On a host-only sequence it is a state change, the cap check
 * included.
 *
 * sunsky_sequence_get_irradiance_frame_table returns the P x n_z x n_phi values sky_{k,p}(c_ij) of
 * frame k, unweighted and not multiplied by omega, with the writing convention of
 * sunsky_sequence_get_irradiance_table: bit for bit the SKY table of the one-frame, weight-1
 * sequence.  It needs prepare_irradiance alone and works on host-only sequences (computed on the
 * host there, on the device otherwise; host-synchronous).
 *
 * sunsky_sequence_irradiance_series is a hot-path call: stream-ordered, no allocation, no
 * host-synchronous call, capturable.  Frame k of [first_frame, first_frame + n_frames) and plane p
 * go to out + ((k - first_frame) P + p) * out_stride.  horizon == NULL is the open horizon and
 * ignores n_sectors, n_profiles and horizon_stride.  n == 0 or n_frames == 0 succeeds (nothing
 * else is looked at); n < 2^32.  Refused with SUNSKY_ERROR_INVALID_VALUE and a message, in this
 * order: a NULL normal or out; n >= 2^32; a sequence without prepare_irradiance_series;
 * first_frame < 0, n_frames < 0 or first_frame + n_frames > count; with a horizon, n_sectors < 1
 * or not a divisor of n_phi, n_profiles other than 1 and n, horizon_stride < n with
 * n_profiles == n and n_sectors > 1; out_stride < n with more than one output plane; a host-only
 * sequence, as for the other launches. */
int sunsky_sequence_prepare_irradiance_series(sunsky_sequence *seq);
int sunsky_sequence_get_irradiance_frame_table(const sunsky_sequence *seq, int k, float *out, size_t capacity,
                                               size_t *count);
int sunsky_sequence_irradiance_series(const sunsky_sequence *seq, sunsky_vec3_in normal, const float *horizon,
                                      int n_sectors, size_t n_profiles, size_t horizon_stride,
                                      const uint8_t *active, size_t n, int first_frame, int n_frames,
                                      float *out, size_t out_stride, void *stream);

/* Gradients of the irradiance with respect to the receiver normals and the frame weights
 * (reverse mode).  Notation as above, with A_p[i, j] = fp32(omega R_p[i, j]) and
 * B_k[p] = fp32(w_k F_k[p]) (the staged image's values, rounded once at prepare time),
 * P = n_planes, Q = n_z n_phi, K = count, a cotangent d_out[p, r] in the layout of
 * sunsky_sequence_irradiance's out (a row stride d_stride is allowed) and
 *     L = sum_r sum_p d_out[p, r] E_p(n_r).
 * E is piecewise linear in n and linear in w, so both gradients are closed forms over the tables.
 * Gradients with respect to a frame's turbidity and sun direction are out of scope: they need a
 * tangent of the 4 x 16 flux rule, which is not defined.
 *
 * Normal gradient: per receiver, written (not accumulated), three world-space planes.
 *     g_l(r) = sum_i sum_j a_r[i, j] c_ij [n_l . c_ij > 0] + sum_k b_r[k] s_k [n_l . s_k > 0],
 *     a_r[i, j] = sum_p d_out[p, r] A_p[i, j],   b_r[k] = sum_p d_out[p, r] B_k[p],
 *     grad_normal(r) = (to_local's linear part)^T g_l(r).
 * The clamp's derivative is the strict step: a dot product of exactly 0 (or a NaN) contributes 0.
 * The dot product is the forward's, fma(a.z, b.z, fma(a.y, b.y, a.x b.x)).  Summation order (the
 * contract; independent of n, of the grid and of the lane), per component of g_l: per record the
 * plane fold a = fma(d_out[p], value_p, a) from 0 in plane order, then fma(a or 0, direction,
 * sum); a row's cells in column order into a row sum that starts at 0; the row sums in row order
 * (row 0 first); then the suns of the staged image in frame order (frames whose w_k F_k is 0 in
 * every plane are not in it).  The sequential depth is n_phi + n_z + count + n_planes fp32
 * additions per component.  Inactive lanes (mask) get exact zeros.
 *
 * Weight gradient: accumulated (+=) into grad_weight[K], as sunsky_sequence_eval_vjp does.
 *     grad_weight[k] += sum_r sum_p d_out[p, r] E^k_p(n_r),
 *     E^k_p(n) = sum_ij omega sky_{k,p}(c_ij) max(0, n_l . c_ij) + F_k[p] max(0, n_l . s_k),
 * sky_{k,p} frame k's term of R_p (reference precision, the disc branch off; spectral: the
 * two-node lerp, an invalid wavelength a plane of zeros) and F_k the unweighted flux.  Every
 * frame counts: one with w_k = 0 gets E^k (not 0), and so does one the forward's image leaves out
 * because w_k F_k = 0.  A frame whose sun is below the horizon gets exactly 0; inactive lanes add
 * exactly 0.  It is computed through the adjoint image, never as n x Q x K work:
 *     G_p[i, j] = sum_r d_out[p, r] max(0, n_l,r . c_ij),   H_p[k] = sum_r d_out[p, r] max(0, n_l,r . s_k),
 *     grad_weight[k] += omega sum_p sum_ij G_p[i, j] sky_{k,p}(c_ij) + sum_p H_p[k] F_k[p].
 * The reduction is deterministic (no float atomics; two runs and any launch shape give the same
 * bits) and its shape is fixed by (n, P, Q, K) and the workspace bound alone -- the grid, the CU
 * count and SUNSKY_AMD_BLOCKS_PER_CU do not enter:
 *   - The receivers are cut into slices.  slices_wanted = ceil(n / 1024), at most 64 and at most
 *     floor(bound / (P (Q + K))) (at least 1); slice_len = ceil(n / slices_wanted) rounded up to a
 *     multiple of 256; slices = ceil(n / slice_len), slice s = receivers [s slice_len, ..).
 *   - Within a slice, per entry (cell or sun) and plane: chunks of 256 consecutive receivers;
 *     a chunk's receivers in index order into a chunk sum that starts at 0,
 *     fma(d_out[p, r], max(0, n_l,r . dir), chunk); the chunk sums in chunk order into the slice's
 *     sum.  One workspace row of P (Q + K) floats per slice.
 *   - The rows are added in slice order: ((row_0 + row_1) + row_2) + ...
 *   - Per frame, 256 lanes: lane l adds its cells (cell = l + 256 t, t ascending) into one sum
 *     that starts at 0, fma(G_p[cell], sky_{k,p}(cell), sum) -- RGB: a cell's three planes in
 *     plane order; spectral: plane by plane, invalid wavelengths skipped --; the 64 lanes of a wave
 *     by the fixed tree (lane l += lane l + off for off = 32, 16, .., 1); the 4 waves in wave
 *     order; times omega; plus h, h = fma(H_p[k], F_k[p], h) from 0 in plane order.
 * The sequential depth is m = 256 + slice_len / 256 + slices + P ceil(Q / 256) + P + 11 fp32
 * additions (chunk, chunks, slices, lane, tree 6 + waves 3 + omega and h 2, suns).
 *
 * sunsky_sequence_prepare_irradiance_grad (host-synchronous; needs prepare_irradiance first)
 * stages on the device what the forward's image lacks -- every frame's local sun direction, the
 * unweighted F_k[p] and every frame's sun column j_k -- and allocates the reduction workspace:
 * at most 64 rows of P (Q + K) floats and at most 2^22 floats (16 MiB), or one row where that is
 * more.  The environment
 * variable SUNSKY_AMD_IRRADIANCE_GRAD_WORKSPACE_FLOATS, read at prepare time, lowers the 2^22.
 * It is sticky: once called, a later prepare_irradiance restages it for the new tables;
 * sunsky_sequence_update drops it together with the tables (prepare_irradiance brings both back).
 * On a host-only sequence it is a state change only.
 *
 * sunsky_sequence_irradiance_vjp is a hot-path call: stream-ordered, no allocation, no
 * host-synchronous call, capturable.  Either output may be NULL (grad_normal: all three planes);
 * d_out must not be NULL; n == 0 succeeds and writes nothing; n <= 2^32 - 256.  Before
 * prepare_irradiance_grad it fails with SUNSKY_ERROR_INVALID_VALUE and a message naming the
 * missing call; a host-only sequence refuses it as the other launches do.  Calls on one sequence
 * share the workspace: ordering them across streams is the caller's job. */
int sunsky_sequence_prepare_irradiance_grad(sunsky_sequence *seq);
int sunsky_sequence_irradiance_vjp(const sunsky_sequence *seq, sunsky_vec3_in normal, const uint8_t *active,
                                   size_t n, const float *d_out, size_t d_stride, sunsky_vec3_out grad_normal,
                                   float *grad_weight, void *stream);

/* Gradients of the irradiance under a horizon profile (reverse mode): with respect to the receiver
 * normals, the frame weights and the profile itself.  Additive: sunsky_sequence_irradiance_vjp and
 * its bits are untouched.  Notation is that of sunsky_sequence_irradiance_horizon and of
 * sunsky_sequence_irradiance_vjp: A_p = fp32(omega R_p) and B_k[p] = fp32(w_k F_k[p]) the staged
 * image's values, n_l = to_local(n), t_r[i, b] = fma(-h_r[b], (float)n_z, (float)(i + 1)),
 * v = min(max(t, 0), 1), dot the forward's fma(z, z, fma(y, y, x x)), a_r and b_r
 * sunsky_sequence_irradiance_vjp's plane folds (from 0, in plane order), and
 *     L = sum_r sum_p d_out[p, r] E_p(n_r; h_r).
 *
 * Normal gradient: written, world space, three planes.
 *     g_l(r) = sum_ij m_r[i, j] c_ij + sum_k [s_k.z >= h_r[b_k]] [n_l . s_k > 0] b_r[k] s_k,
 *     m_r[i, j] = [n_l . c_ij > 0] ? fp32(a_r[i, j] v_r[i, b(j)]) : 0,
 *     grad_normal(r) = (to_local's linear part)^T g_l(r).
 * The step is strict; the sun's visibility is the forward's exact fp32 comparison.  Summation
 * order: sunsky_sequence_irradiance_vjp's (a row's cells in column order into a row sum from 0,
 * the rows in row order, then the image's suns in frame order, every product-and-add one fma);
 * the only addition is the rounded a v.
 *
 * Weight gradient: accumulated (+=), every frame counts (a zero-weight one included).
 *     grad_weight[k] += sum_r sum_p d_out[p, r] E^k_p(n_r; h_r),
 *     E^k_p(n; h) = sum_ij omega sky_{k,p}(c_ij) fp32(max(0, dot) v) + [s_k.z >= h[b_k]] F_k[p] max(0, n_l . s_k),
 * the series' per-frame irradiance under a horizon.  It goes through the adjoint image
 *     G_p[i, j] = sum_r d_out[p, r] fp32(max(0, dot) v_r[i, b(j)]),
 *     H_p[k]    = sum_r d_out[p, r] [s_k.z >= h_r[b_k]] max(0, dot)     for all K frames,
 * b_k from every frame's column j_k, and then through sunsky_sequence_irradiance_vjp's fold,
 * unchanged.  The reduction shape is exactly sunsky_sequence_irradiance_vjp's (slices, chunks of
 * 256 receivers in index order, slice order, the per-frame fold): a function of (n, P, Q, K) and
 * the workspace bound alone, deterministic, no float atomics; which lane or workgroup owns an
 * entry does not enter the bits (H and the profile's layout do not change the shape either).
 *
 * Horizon gradient: written, one value per (sector, receiver) at
 * grad_horizon[b * grad_horizon_stride + r], also for a shared profile (n_profiles = 1): the call
 * does no reduction over receivers, and the caller sums the columns for a shared profile.
 *     dE/dh_r[b] = -(float)n_z sum_i [0 < t_r[i, b] < 1] sum_{j in b} max(0, n_l . c_ij) a_r[i, j].
 * The visible share is linear in h, so E is piecewise linear in h.  In fp32 at most one row per
 * sector has 0 < t < 1 (t_i < 1 implies the exact x + i + 1 < 1, so with t_i > 0 the exact
 * x + i + 2 > 1 and t_{i+1} >= 1): the value is that row's sector cells in column order,
 * s = fma(max(0, dot), a, s) from 0, then s (-(float)n_z); +0 when no row is partly covered.  The
 * sun is a point source: its visibility is a step and contributes no horizon gradient.
 *
 * Consequences.  h <= 0 in every sector (0, -0, -1): grad_normal and grad_weight are bit for bit
 * sunsky_sequence_irradiance_vjp's, grad_horizon is exact zeros.  h > 1 in every sector:
 * grad_normal and grad_horizon are exact zeros, grad_weight is left bit for bit as it was.  A shared
 * profile gives the bits of the same profile repeated per receiver, for all three outputs.
 * Inactive lanes write exact zeros to grad_normal and grad_horizon and add exactly 0 to the
 * weights.  A NaN in a profile is unspecified for that receiver's grad_normal and grad_horizon
 * only, and for the whole grad_weight.  The result does not depend on n, the grid, the lane or
 * SUNSKY_AMD_BLOCKS_PER_CU.
 *
 * There is no new prepare call: sunsky_sequence_prepare_irradiance_grad additionally stages every
 * frame's sun column j_k on the device, under its sticky / restage / update rules.  The call
 * shares sunsky_sequence_irradiance_vjp's workspace; ordering calls on one sequence across
 * streams is the caller's job.
 *
 * A hot-path call: stream-ordered, no allocation, no host-synchronous call, capturable.  Any
 * output may be NULL (grad_normal: all three planes).  n == 0 succeeds and writes nothing (nothing
 * else is looked at); n <= 2^32 - 256.  Refused with SUNSKY_ERROR_INVALID_VALUE and a message, in
 * this order: a NULL normal or d_out; a partly NULL grad_normal; n > 2^32 - 256; a NULL horizon;
 * n_sectors < 1; n_profiles other than 1 and n; horizon_stride < n with n_profiles == n and
 * n_sectors > 1; grad_horizon_stride < n with n_sectors > 1 and a grad_horizon; a sequence without
 * prepare_irradiance or prepare_irradiance_grad (the message names the missing call); n_sectors
 * not a divisor of n_phi; a host-only sequence, as for the other launches; d_stride < n with more
 * than one plane. */
int sunsky_sequence_irradiance_horizon_vjp(const sunsky_sequence *seq, sunsky_vec3_in normal, const float *horizon,
                                           int n_sectors, size_t n_profiles, size_t horizon_stride,
                                           const uint8_t *active, size_t n, const float *d_out, size_t d_stride,
                                           sunsky_vec3_out grad_normal, float *grad_weight, float *grad_horizon,
                                           size_t grad_horizon_stride, void *stream);

/* A caller of sample_direction / pdf_direction / eval: the sun-and-sky light a
 * smooth-diffuse point receives, gathered as the path integrator does at one vertex
 * (src/integrators/path.cpp:176-250; src/bsdfs/diffuse.cpp:100-180): emitter
 * sampling + cosine-hemisphere BSDF sampling combined with the power heuristic, spp
 * samples per point from PCG32Sampler-seeded streams (src/render/sampler.cpp:125-144:
 * sample_tea_32(seed, point index)), each sample drawing next_2d (emitter), next_1d
 * (sample_1, unused by this BSDF) and next_2d (BSDF) as path.cpp:216-234 does.
 * normal: unit world-space normals; reflectance: gray per point (NULL = 1).
 * out planes: 3 (RGB) or n_wavelengths <= 4 (spectral, per-point wavelengths).
 * visibility: NULL for unoccluded points, else one byte per (sample s, point i) at
 * visibility[s * vis_stride + i] with the caller's tracer verdicts on the rays
 * sunsky_direct_diffuse_rays wrote for the same (seed, spp, normal): bit 0 = the
 * shadow ray along the emitter sample is unoccluded (path.cpp:216-219 ray_test),
 * bit 1 = the BSDF ray escapes to the environment (path.cpp:176-196).
 * n < 2^32. */
int sunsky_direct_diffuse(const sunsky_emitter *e, sunsky_vec3_in normal, const float *reflectance,
                          const float *wavelengths, int n_wavelengths, size_t wl_stride, uint32_t seed,
                          uint32_t spp, const uint8_t *visibility, size_t vis_stride, size_t n, float *out,
                          size_t out_stride, void *stream);
/* The rays a wavefront caller traces between the two halves of sunsky_direct_diffuse
 * (the shadow ray of the emitter sample, path.cpp:216-219, and the BSDF ray,
 * path.cpp:176-196), from the same streams and arithmetic as that call: for sample s
 * of point i, emitter_dir[s * ray_stride + i] is the world direction of the emitter
 * sample ((0,0,0) when the sample contributes nothing: pdf 0 or below the point's
 * horizon) and bsdf_dir[s * ray_stride + i] the cosine-sampled world direction
 * ((0,0,0) when its pdf is 0).  ray_stride >= n; n < 2^32. */
int sunsky_direct_diffuse_rays(const sunsky_emitter *e, sunsky_vec3_in normal, uint32_t seed, uint32_t spp,
                               size_t n, sunsky_vec3_out emitter_dir, sunsky_vec3_out bsdf_dir,
                               size_t ray_stride, void *stream);

/* A caller with a glossy vertex: the light a rough conductor (src/bsdfs/roughconductor.cpp,
 * Beckmann or GGX, visible-normal sampling, include/mitsuba/render/microfacet.h)
 * reflects towards wi, gathered as path.cpp:176-250 does at one vertex: per sample the
 * emitter sample (next_2d) weighted by f cos / pdf and the power heuristic, sample_1
 * (next_1d, unused by this BSDF), then the BSDF sample (next_2d): reflected direction,
 * weight F G1(wo), its escaped ray through eval() and pdf_direction().
 * normal, wi: unit world vectors (wi towards the viewer, si.wi in world space).
 * eta, k: complex IOR per RGB channel (3 values); spectral emitters use eta[0], k[0]
 * for every wavelength.  alpha: roughness (clamped to 1e-4 as the reference).
 * visibility: as sunsky_direct_diffuse, for the rays of sunsky_direct_conductor_rays. */
#define SUNSKY_MICROFACET_BECKMANN 0
#define SUNSKY_MICROFACET_GGX 1
int sunsky_direct_conductor(const sunsky_emitter *e, sunsky_vec3_in normal, sunsky_vec3_in wi, int distribution,
                            float alpha, const float *eta, const float *k, const float *wavelengths,
                            int n_wavelengths, size_t wl_stride, uint32_t seed, uint32_t spp,
                            const uint8_t *visibility, size_t vis_stride, size_t n, float *out,
                            size_t out_stride, void *stream);
/* The shadow rays and BSDF rays of sunsky_direct_conductor's samples (same streams and
 * arithmetic): (0,0,0) where the emitter sample contributes nothing (pdf 0 or f cos = 0)
 * or the BSDF sample is invalid.  bsdf_weight (NULL to skip; then eta / k may be NULL):
 * the BSDF sample's weight F(wi.m) G1(wo, m) (roughconductor.cpp sample(), the path
 * throughput factor of a multi-bounce caller) at bsdf_weight[(c * spp + s) * ray_stride + i]
 * for c < 3 (RGB) or c < 1 (spectral: eta[0], k[0]), 0 where the sample is invalid.
 * ray_stride >= n; n < 2^32. */
int sunsky_direct_conductor_rays(const sunsky_emitter *e, sunsky_vec3_in normal, sunsky_vec3_in wi,
                                 int distribution, float alpha, const float *eta, const float *k, uint32_t seed,
                                 uint32_t spp, size_t n, sunsky_vec3_out emitter_dir, sunsky_vec3_out bsdf_dir,
                                 float *bsdf_weight, size_t ray_stride, void *stream);
/* The same two calls with an anisotropic distribution: roughconductor's alpha_u / alpha_v
 * (microfacet.h:92-95, eval :186-207, smith_g1 :330-354, the visible-normal stretch
 * :301-316), alpha_u along the shading frame's first tangent (coordinate_system(normal),
 * include/mitsuba/core/vector.h:116-137) and alpha_v along the second; each clamped to
 * 1e-4.  alpha_u == alpha_v gives the isotropic calls' results bit for bit. */
int sunsky_direct_conductor_aniso(const sunsky_emitter *e, sunsky_vec3_in normal, sunsky_vec3_in wi,
                                  int distribution, float alpha_u, float alpha_v, const float *eta, const float *k,
                                  const float *wavelengths, int n_wavelengths, size_t wl_stride, uint32_t seed,
                                  uint32_t spp, const uint8_t *visibility, size_t vis_stride, size_t n, float *out,
                                  size_t out_stride, void *stream);
int sunsky_direct_conductor_rays_aniso(const sunsky_emitter *e, sunsky_vec3_in normal, sunsky_vec3_in wi,
                                       int distribution, float alpha_u, float alpha_v, const float *eta,
                                       const float *k, uint32_t seed, uint32_t spp, size_t n,
                                       sunsky_vec3_out emitter_dir, sunsky_vec3_out bsdf_dir, float *bsdf_weight,
                                       size_t ray_stride, void *stream);

/* ------------------------------------------------ forward-mode derivatives */
typedef enum sunsky_param {         /* Differentiable traverse() parameters, sunsky.cpp:220-240 */
    SUNSKY_PARAM_TURBIDITY = 0,     /* tangent: 1 value                               */
    SUNSKY_PARAM_ALBEDO = 1,        /* tangent: 1 value or one per channel (3 / 11)   */
    SUNSKY_PARAM_SUN_DIRECTION = 2  /* tangent: 3 values, world space (m_sun_dir)     */
} sunsky_param;
/* eval(si) and its forward-mode derivative along `tangent` of `param`: what
 * dr::enable_grad(param); dr::set_grad(param, tangent); dr::forward_from(param);
 * dr::grad(eval(si)) computes in the reference's AD variants (exercised by
 * sunsky-testing/traversal_test.py:94-145).  Layout as sunsky_eval; d_out has the
 * planes of out.  The tangent of the staged tables is staged by a device kernel
 * (fp64, stream-ordered on `stream`) when the emitter or the tangent changed, then the
 * rays are processed on `stream`. */
int sunsky_eval_jvp(const sunsky_emitter *e, int param, const float *tangent, int tangent_count,
                    sunsky_vec3_in wi, const float *wavelengths, int n_wavelengths, size_t wl_stride,
                    const uint8_t *active, size_t n, float *out, float *d_out, size_t out_stride,
                    void *stream);
/* Reverse mode: grad[p] += sum over rays and output planes of d_out * d eval / d p,
 * i.e. the parameter gradients dr.backward(dr.sum(d_out * eval(si))) accumulates in the
 * reference.  `grad` is a DEVICE array of SUNSKY_GRAD_COUNT floats:
 *   [SUNSKY_GRAD_TURBIDITY]          turbidity
 *   [SUNSKY_GRAD_ALBEDO + c]         albedo of channel c (c < 3 RGB, < 11 spectral;
 *                                    a uniform albedo's gradient is their sum)
 *   [SUNSKY_GRAD_SUN_DIRECTION + k]  sun_direction, world axis k (0 in time/location mode)
 * Accumulation is deterministic (fixed-order workgroup and block reductions). */
#define SUNSKY_GRAD_COUNT 16
#define SUNSKY_GRAD_TURBIDITY 0
#define SUNSKY_GRAD_ALBEDO 1
#define SUNSKY_GRAD_SUN_DIRECTION 12
int sunsky_eval_vjp(const sunsky_emitter *e, sunsky_vec3_in wi, const float *wavelengths, int n_wavelengths,
                    size_t wl_stride, const uint8_t *active, size_t n, const float *d_out, size_t out_stride,
                    float *grad, void *stream);
/* Derivatives of eval(si) with respect to its per-ray input si.wi -- what Dr.Jit traces
 * through eval (sunsky.cpp:303-352) for a differentiable wi.  The function differentiated is
 * eval as written: wo = to_world^-1(-wi) (linear part), cos theta = wo.z,
 * gamma = unit_angle(sun, wo); nothing is renormalised, so the derivative has a radial
 * component.  Masks (horizon, sun-disc test, elevation segment, wavelength validity) are not
 * differentiated.  Inactive lanes (mask, cos theta < 0) and invalid wavelengths give exact
 * zeros in every output.  Reference precision.  Layout and validation as sunsky_eval /
 * sunsky_eval_jvp.  Both calls read only the emitter's device state: they are hot-path calls
 * (stream-ordered, no allocation, no host-synchronous call, capturable).
 *
 * Forward: out = eval(si), d_out = (d eval / d wi) . d_wi, planes as out. */
int sunsky_eval_jvp_dir(const sunsky_emitter *e, sunsky_vec3_in wi, sunsky_vec3_in d_wi,
                        const float *wavelengths, int n_wavelengths, size_t wl_stride,
                        const uint8_t *active, size_t n, float *out, float *d_out,
                        size_t out_stride, void *stream);
/* Reverse: grad_wi[ray] = sum over output planes of d_out * d eval / d wi (3 planes of n,
 * overwritten, not accumulated; per ray, no reduction). */
int sunsky_eval_vjp_dir(const sunsky_emitter *e, sunsky_vec3_in wi,
                        const float *wavelengths, int n_wavelengths, size_t wl_stride,
                        const uint8_t *active, size_t n, const float *d_out,
                        size_t out_stride, sunsky_vec3_out grad_wi, void *stream);
/* The tangent of the staged tables along `tangent` of `param` -- what dr::forward_from(param)
 * propagates into compute_radiance_params / compute_sun_params (sunsky.h:158-231, 404-419)
 * before eval: SUNSKY_TANGENT_FLOATS floats, d{A..I, rad} of channel c at c * 10 (+ q), the
 * local sun direction's tangent at 110..112, the sun table's at 128.  on_device = 1 stages
 * them with the kernel eval_jvp uses (blocking, on the null stream), 0 on the host (also
 * for host-only emitters); both compute the same fp64 arithmetic. */
#define SUNSKY_TANGENT_FLOATS (128 + 3240)
int sunsky_emitter_tangent_tables(const sunsky_emitter *e, int param, const float *tangent, int tangent_count,
                                  int on_device, float *out, size_t capacity, size_t *count);

/* --------------------------------------------- dataset I/O (sunsky_v.cpp:16-18) */
/* array_from_file_d / _f (sunsky.h:516-561): file_dtype 0 = infer, 1 = fp32, 2 = fp64.
 * Writes min(count, capacity) fp64 values; shape gets up to 16 dims. */
int sunsky_array_from_file(const char *path, int file_dtype, double *out, size_t capacity,
                           size_t *count, uint64_t *shape, int *ndims);
/* array_to_file (sunsky.h:573-597) */
int sunsky_array_to_file(const char *path, const float *data, size_t count, const uint64_t *shape,
                         int ndims);
/* mi.hosek_sun_rad (sunsky_v.cpp:19): arhosekskymodel_solar_radiance_internal2
 * (ArHosekSkyModel.c:686-784), the Hosek-Wilkie solar radiance in fp64 for a
 * turbidity, a wavelength (nm), the sun elevation and the angle gamma from the sun
 * centre (radians).  dataset_path: NULL for the bundled pack. */
int sunsky_hosek_sun_rad(const char *dataset_path, double turbidity, double wavelength, double elevation,
                         double gamma, double *out);

/* Plugin identification of MI_EXPORT_PLUGIN (class.h:220-225; sunsky.cpp:1037):
 * plugin_name() = "sunsky". */
const char *plugin_name(void);
const char *plugin_descr(void);

/* Path of the bundled dataset pack the library resolves by default. */
int sunsky_default_dataset_path(char *buf, size_t capacity);

/* ------------------------------------------------------------ multi-GPU gather
 * configs[4]: one process per GPU, each evaluating its contiguous
 * slice of the ray batch; the only exchange is the gather of the radiance planes to
 * one rank (the reference's ncclGather, rccl.h:745-746).  RCCL is loaded on first use
 * (dlopen librccl.so.1); without it these calls return SUNSKY_ERROR_COMM. */
#define SUNSKY_COMM_ID_BYTES 128
typedef struct sunsky_comm sunsky_comm;
/* ncclGetUniqueId: rank 0 makes the id, the caller hands it to every rank (any channel). */
int sunsky_comm_get_unique_id(unsigned char id[SUNSKY_COMM_ID_BYTES]);
/* ncclCommInitRank on the CURRENT HIP device (collective over the nranks processes). */
int sunsky_comm_create(const unsigned char id[SUNSKY_COMM_ID_BYTES], int nranks, int rank, sunsky_comm **out);
void sunsky_comm_destroy(sunsky_comm *comm);
int sunsky_comm_info(const sunsky_comm *comm, int *rank, int *nranks, int *device);
/* Gather every rank's shard into root's final planes, stream-ordered: rank r sends nplanes
 * planes of counts[r] floats (plane p at send + p * send_stride); on root they land at
 * recv + p * recv_stride + sum(counts[0..r)).  counts[] (nranks entries) is the same on
 * every rank; recv is only read on root.  Grouped ncclSend / ncclRecv: no padding and no
 * re-layout copy; root's own shard is a device copy (none when already in place). */
int sunsky_gather_radiance(sunsky_comm *comm, int root, const float *send, size_t send_stride, int nplanes,
                           const size_t *counts, float *recv, size_t recv_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SUNSKY_AMD_H */
