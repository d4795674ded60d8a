"""ctypes front-end of the CPU oracle -- TEST INFRASTRUCTURE ONLY.

Loaded by tests/, bench.py (cpu_baseline leg) and __graft_entry__.smoke()
as the parity checker.  The product package never imports this module.

Scene dictionaries use the reference plugin's parameter names and defaults
(sunsky.cpp:889-948); ``variant`` is "rgb" | "spectral" and ``semantics`` is
"jit" (llvm_/cuda_ variants) | "scalar" (scalar_ variants).
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "build", "libsunsky_oracle.so")
PACK_PATH = os.path.join(HERE, "..", "mitsuba3-sunsky_amd", "data", "sunsky_datasets.pack")

WAVELENGTH_NODES = np.arange(320, 721, 40, dtype=np.float32)
TIME_LOCATION_KEYS = ("latitude", "longitude", "timezone", "year", "month", "day",
                      "hour", "minute", "second")


class _Params(C.Structure):
    _fields_ = [
        ("spectral", C.c_int), ("jit_semantics", C.c_int),
        ("turbidity", C.c_float), ("sky_scale", C.c_float), ("sun_scale", C.c_float),
        ("sun_aperture_deg", C.c_float),
        ("albedo_n", C.c_int), ("albedo", C.c_float * 11),
        ("use_sun_direction", C.c_int), ("sun_direction", C.c_float * 3),
        ("latitude", C.c_float), ("longitude", C.c_float), ("timezone", C.c_float),
        ("year", C.c_int), ("month", C.c_int), ("day", C.c_int),
        ("hour", C.c_float), ("minute", C.c_float), ("second", C.c_float),
        ("to_world", C.c_float * 16),
        ("bsphere_center", C.c_float * 3), ("bsphere_radius", C.c_float),
    ]


class _Info(C.Structure):
    _fields_ = [
        ("sun_dir_world", C.c_double * 3), ("sun_dir_local", C.c_double * 3),
        ("sun_angles", C.c_double * 2), ("frame_s", C.c_double * 3), ("frame_t", C.c_double * 3),
        ("sun_eta", C.c_double), ("w_sky", C.c_double), ("area_ratio", C.c_double),
        ("cos_cutoff", C.c_double), ("nb_channels", C.c_int),
        ("sky_params", C.c_double * 99), ("sky_radiance", C.c_double * 11),
        ("gaussians", C.c_double * 100), ("gauss_cdf", C.c_double * 20), ("gauss_sum", C.c_double),
        ("spec_pdf", C.c_double * 10), ("spec_cdf", C.c_double * 9), ("spec_integral", C.c_double),
        ("spec_size", C.c_int),
    ]


_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = C.CDLL(LIB_PATH)
        _lib.oracle_last_error.restype = C.c_char_p
        _lib.oracle_hw_sun_radiance_f32.restype = C.c_float
        _lib.oracle_hw_sun_radiance_f32.argtypes = [C.c_void_p] + [C.c_float] * 4
        _lib.oracle_hw_sun_radiance_f64.restype = C.c_double
        _lib.oracle_hw_sun_radiance_f64.argtypes = [C.c_void_p] + [C.c_double] * 4
        _lib.oracle_sun_segment_f32.restype = C.c_int
        _lib.oracle_sun_segment_f32.argtypes = [C.c_float]
        _lib.oracle_check_sun_segment_thresholds.restype = C.c_long
        _lib.oracle_check_sun_segment_thresholds.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        _lib.oracle_sun_table_f32.restype = C.c_size_t
        _lib.oracle_sun_table_f64.restype = C.c_size_t
    return _lib


def albedo_values(albedo, spectral):
    """Texture::eval of the albedo at the model channels (extract_albedo,
    sunsky.cpp:956-978): uniform float, per-channel list, or an 'irregular'
    spectrum dict (linear interpolation, zero outside its range)."""
    nch = 11 if spectral else 3
    if isinstance(albedo, dict):
        if albedo.get("type") != "irregular":
            raise ValueError("only 'irregular' spectra are supported as albedo textures")
        if not spectral:
            raise ValueError("irregular albedo spectra are only supported in spectral variants")
        wl = np.array([float(v) for v in str(albedo["wavelengths"]).split(",")], dtype=np.float64)
        vals = np.array([float(v) for v in str(albedo["values"]).split(",")], dtype=np.float64)
        out = np.interp(WAVELENGTH_NODES.astype(np.float64), wl, vals, left=0.0, right=0.0)
        return out.astype(np.float32)
    arr = np.atleast_1d(np.asarray(albedo, dtype=np.float32))
    if arr.size == 1:
        return np.full(nch, arr[0], dtype=np.float32)
    if arr.size != nch:
        raise ValueError(f"albedo needs 1 or {nch} values, got {arr.size}")
    return arr


def make_params(d, variant="rgb", semantics="jit"):
    p = _Params()
    spectral = variant == "spectral"
    p.spectral = int(spectral)
    p.jit_semantics = int(semantics == "jit")
    p.turbidity = d.get("turbidity", 3.0)
    p.sky_scale = d.get("sky_scale", 1.0)
    p.sun_scale = d.get("sun_scale", 1.0)
    p.sun_aperture_deg = d.get("sun_aperture", 0.5358)
    alb = albedo_values(d.get("albedo", 0.3), spectral)
    p.albedo_n = len(alb)
    for i, v in enumerate(alb):
        p.albedo[i] = float(v)
    if "sun_direction" in d:
        if any(k in d for k in TIME_LOCATION_KEYS):
            raise ValueError("Both the 'sun_direction' and parameters for time/location were provided")
        p.use_sun_direction = 1
        for i in range(3):
            p.sun_direction[i] = float(d["sun_direction"][i])
    p.latitude = d.get("latitude", 35.6894)
    p.longitude = d.get("longitude", 139.6917)
    p.timezone = d.get("timezone", 9.0)
    p.year = int(d.get("year", 2010))
    p.month = int(d.get("month", 7))
    p.day = int(d.get("day", 10))
    p.hour = d.get("hour", 15.0)
    p.minute = d.get("minute", 0.0)
    p.second = d.get("second", 0.0)
    m = np.asarray(d.get("to_world", np.eye(4)), dtype=np.float32).reshape(4, 4)
    for i in range(16):
        p.to_world[i] = float(m.flat[i])
    c = d.get("bsphere_center", (0.0, 0.0, 0.0))
    for i in range(3):
        p.bsphere_center[i] = float(c[i])
    p.bsphere_radius = d.get("bsphere_radius", 1.0)
    return p


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Oracle:
    """One staged emitter on the CPU; precision 'f32' (reference fp32 ops) or 'f64'."""

    def __init__(self, scene, variant="rgb", semantics="jit", precision="f32"):
        self.variant, self.semantics, self.precision = variant, semantics, precision
        self.spectral = variant == "spectral"
        self.dtype = np.float32 if precision == "f32" else np.float64
        self._sfx = precision
        L = lib()
        self._p = make_params(scene, variant, semantics)
        h = C.c_void_p()
        rc = getattr(L, f"oracle_create_{precision}")(C.byref(self._p), os.path.abspath(PACK_PATH).encode(), C.byref(h))
        if rc != 0:
            raise ValueError(L.oracle_last_error().decode())
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            try:
                getattr(lib(), f"oracle_destroy_{self._sfx}")(h)
            except Exception:   # interpreter shutdown: the library may already be gone
                pass

    def _fn(self, name):
        return getattr(lib(), f"oracle_{name}_{self._sfx}")

    def info(self):
        inf = _Info()
        self._fn("info")(self._h, C.byref(inf))
        nch = inf.nb_channels
        return {
            "sun_dir_world": np.array(inf.sun_dir_world), "sun_dir_local": np.array(inf.sun_dir_local),
            "sun_angles": np.array(inf.sun_angles), "frame_s": np.array(inf.frame_s),
            "frame_t": np.array(inf.frame_t), "sun_eta": inf.sun_eta, "w_sky": inf.w_sky,
            "area_ratio": inf.area_ratio, "cos_cutoff": inf.cos_cutoff,
            "sky_params": np.array(inf.sky_params[: nch * 9]).reshape(nch, 9),
            "sky_radiance": np.array(inf.sky_radiance[:nch]),
            "gaussians": np.array(inf.gaussians).reshape(20, 5),
            "gauss_cdf": np.array(inf.gauss_cdf), "gauss_sum": inf.gauss_sum,
            "spec_pdf": np.array(inf.spec_pdf[: inf.spec_size]),
            "spec_cdf": np.array(inf.spec_cdf[: max(inf.spec_size - 1, 0)]),
            "spec_integral": inf.spec_integral,
        }

    def sun_table(self):
        out = np.zeros(45 * 3 * 4 * 6, dtype=self.dtype)
        n = self._fn("sun_table")(self._h, _ptr(out), C.c_size_t(out.size))
        return out[:n]

    def eval(self, wi, wavelengths=None):
        """eval(si) with si.wi = wi (n,3).  RGB -> (n,3).  Spectral: wavelengths
        (k, n) or (n,) -> (k, n) (or (n,))."""
        wi = np.asarray(wi, dtype=np.float32)
        n = wi.shape[0]
        wx, wy, wz = _f(wi[:, 0]), _f(wi[:, 1]), _f(wi[:, 2])
        if not self.spectral:
            out = np.zeros((3, n), dtype=self.dtype)
            self._fn("eval")(self._h, _ptr(wx), _ptr(wy), _ptr(wz), None, 0, C.c_size_t(n), _ptr(out))
            return out.T.copy()
        lam = np.asarray(wavelengths, dtype=np.float32)
        squeeze = lam.ndim <= 1
        if lam.ndim == 0:
            lam = np.full((1, n), lam, dtype=np.float32)
        elif lam.ndim == 1:
            lam = lam.reshape(1, n)
        lam = _f(lam)
        k = lam.shape[0]
        out = np.zeros((k, n), dtype=self.dtype)
        self._fn("eval")(self._h, _ptr(wx), _ptr(wy), _ptr(wz), _ptr(lam), k, C.c_size_t(n), _ptr(out))
        return out[0] if squeeze else out

    def sample_direction(self, sample, it_p=None, wavelengths=None):
        sample = np.asarray(sample, dtype=np.float32)
        n = sample.shape[0]
        ux, uy = _f(sample[:, 0]), _f(sample[:, 1])
        px = py = pz = None
        if it_p is not None:
            it_p = np.asarray(it_p, dtype=np.float32)
            px, py, pz = _f(it_p[:, 0]), _f(it_p[:, 1]), _f(it_p[:, 2])
        d = np.zeros((3, n), dtype=self.dtype)
        pdf = np.zeros(n, dtype=self.dtype)
        dist = np.zeros(n, dtype=self.dtype)
        if self.spectral:
            lam = _f(np.asarray(wavelengths, dtype=np.float32).reshape(-1, n))
            k = lam.shape[0]
            if not 1 <= k <= 16:   # the C side's per-sample buffer (kMaxLambdaPerRay)
                raise ValueError(f"1..16 wavelengths per sample, got {k}")
        else:
            lam, k = None, 3
        w = np.zeros((k, n), dtype=self.dtype)
        self._fn("sample_direction")(self._h, _ptr(ux), _ptr(uy), _ptr(px), _ptr(py), _ptr(pz),
                                     _ptr(lam), k if self.spectral else 0, C.c_size_t(n),
                                     _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(pdf), _ptr(dist), _ptr(w))
        return {"d": d.T.copy(), "pdf": pdf, "dist": dist, "weight": w.T.copy()}

    def pdf_direction(self, d):
        d = np.asarray(d, dtype=np.float32)
        n = d.shape[0]
        out = np.zeros(n, dtype=self.dtype)
        self._fn("pdf_direction")(self._h, _ptr(_f(d[:, 0])), _ptr(_f(d[:, 1])), _ptr(_f(d[:, 2])),
                                  C.c_size_t(n), _ptr(out))
        return out

    def sample_ray(self, wavelength_sample, sample2, sample3):
        ws = _f(wavelength_sample)
        s2 = np.asarray(sample2, dtype=np.float32)
        s3 = np.asarray(sample3, dtype=np.float32)
        n = ws.shape[0]
        o = np.zeros((3, n), dtype=self.dtype)
        d = np.zeros((3, n), dtype=self.dtype)
        lam = np.zeros((4, n), dtype=self.dtype)
        k = 4 if self.spectral else 3
        w = np.zeros((k, n), dtype=self.dtype)
        self._fn("sample_ray")(self._h, _ptr(ws), _ptr(_f(s2[:, 0])), _ptr(_f(s2[:, 1])),
                               _ptr(_f(s3[:, 0])), _ptr(_f(s3[:, 1])), C.c_size_t(n),
                               _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(d[0]), _ptr(d[1]), _ptr(d[2]),
                               _ptr(lam), _ptr(w))
        return {"o": o.T.copy(), "d": d.T.copy(), "wavelengths": lam.T.copy(), "weight": w.T.copy()}

    def sample_wavelengths(self, wi, sample):
        """sample_wavelengths(si{wi}, sample) (sunsky.cpp:463-480) -> (lambda (n, 4), weight (n, k))."""
        wi = np.asarray(wi, dtype=np.float32)
        n = wi.shape[0]
        s = _f(sample if sample is not None else np.zeros(n, np.float32))
        lam = np.zeros((4, n), dtype=self.dtype)
        w = np.zeros((4 if self.spectral else 3, n), dtype=self.dtype)
        self._fn("sample_wavelengths")(self._h, _ptr(_f(wi[:, 0])), _ptr(_f(wi[:, 1])), _ptr(_f(wi[:, 2])),
                                       _ptr(s), C.c_size_t(n), _ptr(lam), _ptr(w))
        return lam.T.copy(), w.T.copy()

    def override_w_sky(self, w_sky):
        """Adopt the product's staged sampling weight so sampling parity isolates the kernels."""
        f = self._fn("override_w_sky")
        f.argtypes = [C.c_void_p, C.c_double]
        f(self._h, float(w_sky))

    def override_spectral_distr(self, pdf):
        """Adopt the product's staged wavelength-distribution nodes (sunsky.cpp:870-885) and
        rebuild the CDF with the oracle's compute_cdf (distr_1d.h:513-585), so wavelength
        sampling parity isolates the kernels from the independently staged quadrature."""
        pdf = np.ascontiguousarray(pdf, dtype=np.float64)
        f = self._fn("override_spectral_distr")
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        if f(self._h, _ptr(pdf), int(pdf.size)) != 0:
            raise ValueError(lib().oracle_last_error().decode())

    def adopt_sampling_state(self, em):
        """Adopt everything the product stages from its own quadrature that sampling reads:
        w_sky and (spectral) the wavelength distribution's nodes.  em: a sunsky_amd emitter."""
        self.override_w_sky(em.sky_sampling_w)
        if self.spectral:
            self.override_spectral_distr(em.table("spectral_pdf"))

    def round_staged_tables(self):
        """Round the staged radiance tables to fp32 (the reference's staging precision,
        sunsky.cpp:182-195) and take the fp32 segment decision: with precision 'f64', the exact
        value of the fp32-staged algorithm."""
        self._fn("round_staged_tables")(self._h)

    def adopt_tables(self, em):
        """Evaluate on the product's own staged fp32 tables (sky coefficients, sky radiance,
        sun table, limb darkening), its fp32 local sun direction, disc cutoff and disc area
        ratio, with the fp32 segment decision: with precision 'f64', the exact value of what
        the kernels compute from their inputs, so GPU - this is the kernels' arithmetic error
        alone.  em: a sunsky_amd emitter."""
        t = [np.ascontiguousarray(em.table(k), dtype=np.float32)
             for k in ("sky_params", "sky_radiance", "sun_radiance", "sun_ld")]
        inf = em.info()
        sun = np.ascontiguousarray(inf["sun_dir_local"], dtype=np.float32)
        f = self._fn("adopt_tables")
        f.argtypes = [C.c_void_p] + [C.c_void_p, C.c_size_t] * 4 + [C.c_void_p, C.c_float, C.c_float]
        args = []
        for a in t:
            args += [_ptr(a), a.size]
        if f(self._h, *args, _ptr(sun), C.c_float(inf["cos_cutoff"]), C.c_float(inf["area_ratio"])) != 0:
            raise ValueError(lib().oracle_last_error().decode())

    def hw_sun_radiance(self, turbidity, wavelength, elevation, gamma):
        return self._fn("hw_sun_radiance")(self._h, turbidity, wavelength, elevation, gamma)


def sun_coordinates(year=2010, month=7, day=10, hour=15.0, minute=0.0, second=0.0,
                    latitude=35.6894, longitude=139.6917, timezone=9.0):
    out = (C.c_float * 3)()
    lib().oracle_sun_coordinates(int(year), int(month), int(day), C.c_float(hour), C.c_float(minute),
                                 C.c_float(second), C.c_float(latitude), C.c_float(longitude),
                                 C.c_float(timezone), out)
    return np.array(list(out), dtype=np.float32)


def gauss_legendre(n):
    x = np.zeros(n)
    w = np.zeros(n)
    lib().oracle_gauss_legendre(n, _ptr(x), _ptr(w))
    return x, w


def sun_segment_f32(cos_theta):
    """render_sun's fp32 elevation segment of each cos theta (sunsky.cpp:579-584)."""
    z = np.atleast_1d(np.asarray(cos_theta, np.float32))
    return np.array([lib().oracle_sun_segment_f32(float(v)) for v in z], np.int32)


def check_sun_segment_thresholds(z):
    """(mismatches, first bad fp32 bit pattern or None): every fp32 in [0, 1] through the fp32
    segment decision against the threshold table z[0..44] (OpenMP)."""
    z = np.ascontiguousarray(np.asarray(z, np.float32))
    assert z.shape == (45,)
    first = C.c_uint(0)
    bad = lib().oracle_check_sun_segment_thresholds(z.ctypes.data, C.byref(first))
    return int(bad), (None if first.value == 0xffffffff else int(first.value))


def set_threads(n):
    lib().oracle_set_threads(int(n))


def set_quadrature_sum(sequential):
    """estimate_sky_sun_ratio's 40,000-term sums (sunsky.cpp:815, 849): False (default) adds
    the fp32 terms exactly, True one by one in fp32 (affects Oracles created afterwards)."""
    lib().oracle_set_quadrature_sum(int(bool(sequential)))


def get_threads():
    return lib().oracle_get_threads()


# ---------------------------------------------------------------- caller: direct light at diffuse points
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def sample_tea_32(v0, v1, rounds=4):
    """sample_tea_32, include/mitsuba/core/random.h:77-90 (uint32 arrays)."""
    v0 = np.asarray(v0, dtype=np.uint32).copy()
    v1 = np.asarray(v1, dtype=np.uint32).copy()
    s = np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(rounds):
            s = np.uint32(s + np.uint32(0x9E3779B9))
            v0 += ((v1 << np.uint32(4)) + np.uint32(0xA341316C)) ^ (v1 + s) ^ ((v1 >> np.uint32(5)) + np.uint32(0xC8013EA4))
            v1 += ((v0 << np.uint32(4)) + np.uint32(0xAD90777D)) ^ (v0 + s) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7E95761E))
    return v0, v1


class Pcg32:
    """PCG32 (O'Neill's pcg32_srandom_r / pcg32_random_r), vectorised over lanes, seeded as
    PCG32Sampler::seed (src/render/sampler.cpp:125-144): rng.seed(*sample_tea_32(seed, lane)).
    next_float follows Dr.Jit's next_float32 (23 high bits as a [1, 2) mantissa, minus 1)."""

    MULT = np.uint64(0x5851F42D4C957F2D)

    def __init__(self, seed, n):
        v0, v1 = sample_tea_32(np.full(n, seed, dtype=np.uint32), np.arange(n, dtype=np.uint32))
        self.state = np.zeros(n, dtype=np.uint64)
        self.inc = (v1.astype(np.uint64) << np.uint64(1)) | np.uint64(1)
        self.next_uint32()
        self.state += v0.astype(np.uint64)
        self.next_uint32()

    def next_uint32(self):
        old = self.state
        with np.errstate(over="ignore"):
            self.state = old * self.MULT + self.inc
        xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
        rot = (old >> np.uint64(59)).astype(np.uint32)
        return (xs >> rot) | (xs << ((np.uint32(0) - rot) & np.uint32(31)))

    def next_float(self):
        bits = (self.next_uint32() >> np.uint32(9)) | np.uint32(0x3F800000)
        return bits.view(np.float32) - np.float32(1.0)


def _coordinate_system(n):
    """coordinate_system, include/mitsuba/core/vector.h:116-137 (fp32)."""
    n = n.astype(np.float32)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sgn = np.copysign(np.float32(1), nz).astype(np.float32)      # mulsign uses the sign bit
    a = (np.float32(-1) / (sgn + nz)).astype(np.float32)
    b = (nx * ny * a).astype(np.float32)
    s = np.stack([sgn * (nx * nx * a) + np.float32(1), sgn * b, -sgn * nx], axis=1).astype(np.float32)
    t = np.stack([b, ny * (ny * a) + sgn, -ny], axis=1).astype(np.float32)
    return s, t


def _disk_concentric(sx, sy):
    """square_to_uniform_disk_concentric, include/mitsuba/core/warp.h:54-90 (fp32)."""
    x = (np.float32(2) * sx - np.float32(1)).astype(np.float32)
    y = (np.float32(2) * sy - np.float32(1)).astype(np.float32)
    is_zero = (x == 0) & (y == 0)
    q13 = np.abs(x) < np.abs(y)
    r = np.where(q13, y, x)
    rp = np.where(q13, x, y)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = (np.float32(0.25 * np.pi) * rp / r).astype(np.float32)
    phi = np.where(q13, np.float32(0.5 * np.pi) - phi, phi)
    phi = np.where(is_zero, np.float32(0), phi).astype(np.float32)
    return (r * np.cos(phi)).astype(np.float32), (r * np.sin(phi)).astype(np.float32)


def _mis_power(a, b):
    """mis_weight, src/integrators/path.cpp:315-321."""
    a = a * a
    b = b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        w = a / (a + b)
    return np.where(np.isfinite(w), w, 0.0)


def _direct_diffuse_samples(em, normals, seed, spp, lam):
    """Per sample of direct_diffuse: the emitter sample (sample_direction result, the
    cosine at the point, whether it contributes) and the cosine-sampled BSDF direction
    with its pdf, from the PCG32Sampler streams (u_em = next_2d, sample_1 = next_1d -- unused
    by the diffuse BSDF --, u_bsdf = next_2d; path.cpp:216-234)."""
    normals = np.asarray(normals, dtype=np.float32)
    n = normals.shape[0]
    rng = Pcg32(seed, n)
    s, t = _coordinate_system(normals)
    for _ in range(spp):
        u0, u1 = rng.next_float(), rng.next_float()
        rng.next_float()
        u2, u3 = rng.next_float(), rng.next_float()
        # emitter sampling (path.cpp:208-250)
        r = em.sample_direction(np.stack([u0, u1], axis=1), wavelengths=lam)
        cos_em = (normals.astype(np.float64) * r["d"]).sum(axis=1)
        ok = (r["pdf"] != 0) & (cos_em > 0)
        # BSDF sampling (path.cpp:176-196): square_to_cosine_hemisphere in the normal's frame
        px, py = _disk_concentric(u2, u3)
        lz = np.sqrt(np.maximum(0.0, 1.0 - (px.astype(np.float64) ** 2 + py.astype(np.float64) ** 2)))
        dw = (s * px[:, None] + t * py[:, None] + normals * lz[:, None]).astype(np.float32)
        yield r, cos_em, ok, dw, lz / np.pi


def direct_diffuse(em, normals, seed, spp, wavelengths=None, rho=None, vis=None):
    """Sun-and-sky light at smooth-diffuse points, gathered as the path integrator does at
    one vertex (src/integrators/path.cpp:176-250; diffuse BSDF src/bsdfs/diffuse.cpp:100-180):
    emitter sampling + cosine BSDF sampling with the power heuristic, spp samples per point.
    em: an Oracle.  normals (n, 3); wavelengths (k, n) for spectral.  vis: None or (spp, n)
    uint8 tracer verdicts (bit 0 the shadow ray is unoccluded, path.cpp:216-219; bit 1 the
    BSDF ray escapes, path.cpp:176-196).  Returns (C, n) fp64."""
    normals = np.asarray(normals, dtype=np.float32)
    n = normals.shape[0]
    c = wavelengths.shape[0] if em.spectral else 3
    acc = np.zeros((c, n), dtype=np.float64)
    lam = None if not em.spectral else np.asarray(wavelengths, dtype=np.float32)
    for k, (r, cos_em, ok, dw, bp) in enumerate(_direct_diffuse_samples(em, normals, seed, spp, lam)):
        v = np.full(n, 3, np.uint8) if vis is None else np.asarray(vis[k], dtype=np.uint8)
        ok = ok & ((v & 1) != 0)
        bpdf = np.where(ok, cos_em / np.pi, 0.0)
        scale = np.where(ok, bpdf * _mis_power(r["pdf"], bpdf), 0.0)
        acc += scale[None, :] * r["weight"].T
        # the escaped ray: eval weighted by MIS against pdf_direction
        esc = (bp > 0) & ((v & 2) != 0)
        mis = np.where(esc, _mis_power(bp, em.pdf_direction(dw)), 0.0)
        e = em.eval(-dw, lam) if em.spectral else em.eval(-dw).T
        acc += mis[None, :] * e
    r = np.ones(n) if rho is None else np.asarray(rho, dtype=np.float64)
    return acc * (r / spp)[None, :]


def direct_diffuse_rays(em, normals, seed, spp):
    """The rays a tracer tests for direct_diffuse (sunsky_direct_diffuse_rays): emitter-sample
    directions and BSDF directions, each (spp, n, 3) fp32, zero where no ray is needed."""
    em_d, bs_d = [], []
    for r, cos_em, ok, dw, bp in _direct_diffuse_samples(em, normals, seed, spp, None if not em.spectral else
                                                         np.full((1, len(normals)), 500.0, np.float32)):
        em_d.append(np.where(ok[:, None], r["d"], 0.0).astype(np.float32))
        bs_d.append(np.where((bp > 0)[:, None], dw, 0.0).astype(np.float32))
    return np.stack(em_d), np.stack(bs_d)


# ---------------------------------------------------------------- caller: a rough-conductor vertex
def _auv(a):
    """alpha as (alpha_u, alpha_v): a float is isotropic (microfacet.h:75-78)."""
    if np.ndim(a) == 0:
        return float(a), float(a)
    au, av = a
    return float(au), float(av)


def _mf_eval(distr, a, m):
    """MicrofacetDistribution::eval (include/mitsuba/render/microfacet.h:186-207); a = alpha or
    (alpha_u, alpha_v)."""
    au, av = _auv(a)
    ct2 = m[:, 2] ** 2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if distr == "beckmann":
            r = np.exp(-((m[:, 0] / au) ** 2 + (m[:, 1] / av) ** 2) / ct2) / (np.pi * au * av * ct2 * ct2)
        else:
            r = 1.0 / (np.pi * au * av * ((m[:, 0] / au) ** 2 + (m[:, 1] / av) ** 2 + m[:, 2] ** 2) ** 2)
    r = np.nan_to_num(r, nan=0.0, posinf=0.0)
    return np.where(r * m[:, 2] > 1e-20, r, 0.0)


def _mf_smith_g1(distr, a, v, m):
    """MicrofacetDistribution::smith_g1 (microfacet.h:330-354)."""
    au, av = _auv(a)
    xy = (au * v[:, 0]) ** 2 + (av * v[:, 1]) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t2 = xy / v[:, 2] ** 2
        if distr == "beckmann":
            q = 1.0 / np.sqrt(t2)
            r = np.where(q >= 1.6, 1.0, (3.535 * q + 2.181 * q * q) / (1.0 + 2.276 * q + 2.577 * q * q))
        else:
            r = 2.0 / (1.0 + np.sqrt(1.0 + t2))
    r = np.where(xy == 0.0, 1.0, r)
    return np.where((v * m).sum(axis=1) * v[:, 2] <= 0.0, 0.0, r)


def _mf_sample(distr, a, wi, u):
    """MicrofacetDistribution::sample with visible normals (microfacet.h:293-320, 357-410) -> (m, pdf)."""
    from scipy.special import erf, erfinv
    au, av = _auv(a)
    wp = np.stack([au * wi[:, 0], av * wi[:, 1], wi[:, 2]], axis=1)
    wp /= np.linalg.norm(wp, axis=1, keepdims=True)
    st2 = np.maximum(1.0 - wp[:, 2] ** 2, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sqrt(st2)
        sp, cp = np.clip(wp[:, 1] * inv, -1, 1), np.clip(wp[:, 0] * inv, -1, 1)
    pole = ~(st2 > 0) | ~np.isfinite(inv)
    sp, cp = np.where(pole, 0.0, sp), np.where(pole, 1.0, cp)
    ct = wp[:, 2]
    ux, uy = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
    if distr == "beckmann":
        tan_i = np.sqrt(np.maximum(1.0 - ct * ct, 0.0)) / ct
        with np.errstate(divide="ignore"):
            cot_i = 1.0 / tan_i          # normal incidence: inf, erf(inf) = 1 as dr::rcp gives
        maxval = erf(cot_i)
        ux = np.clip(ux, 1e-6, 1 - 1e-6)
        uy = np.clip(uy, 1e-6, 1 - 1e-6)
        x = maxval - (maxval + 1.0) * erf(np.sqrt(-np.log(ux)))
        ux = ux * (1.0 + maxval + tan_i * np.exp(-cot_i ** 2) / np.sqrt(np.pi))
        for _ in range(3):
            slope = erfinv(x)
            value = 1.0 + x + tan_i * np.exp(-slope ** 2) / np.sqrt(np.pi) - ux
            x = x - value / (1.0 - slope * tan_i)
        sx, sy = erfinv(x), erfinv(2.0 * uy - 1.0)
    else:
        px, py = _disk_concentric(u[:, 0], u[:, 1])
        px, py = px.astype(np.float64), py.astype(np.float64)
        s = 0.5 * (1.0 + ct)
        py = np.sqrt(np.maximum(1.0 - px * px, 0.0)) * (1 - s) + py * s
        pz = np.sqrt(np.maximum(1.0 - (px * px + py * py), 0.0))
        si = np.sqrt(np.maximum(1.0 - ct * ct, 0.0))
        norm = 1.0 / (si * py + ct * pz)
        sx, sy = (ct * py - si * pz) * norm, px * norm
    tx, ty = (cp * sx - sp * sy) * au, (sp * sx + cp * sy) * av
    m = np.stack([-tx, -ty, np.ones_like(tx)], axis=1)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    pdf = _mf_eval(distr, a, m) * _mf_smith_g1(distr, a, wi, m) * np.abs((wi * m).sum(axis=1)) / wi[:, 2]
    return m, pdf


def _fresnel_conductor(c, eta, k):
    """fresnel_conductor (include/mitsuba/render/fresnel.h:93-117)."""
    c2 = c * c
    s2 = 1.0 - c2
    t1 = eta * eta - k * k - s2
    ab = np.sqrt(np.maximum(t1 * t1 + 4.0 * k * k * eta * eta, 0.0))
    a = np.sqrt(np.maximum(0.5 * (ab + t1), 0.0))
    term1, term2 = ab + c2, 2.0 * c * a
    rs = (term1 - term2) / (term1 + term2)
    term3, term4 = ab * c2 + s2 * s2, term2 * s2
    rp = rs * (term3 - term4) / (term3 + term4)
    return 0.5 * (rs + rp)


def _conductor_eval_pdf(distr, a, wi, wo):
    """RoughConductor::eval (without F) and ::pdf (src/bsdfs/roughconductor.cpp:308-420) -> (D G / 4 cos_i, pdf, cos_ih)."""
    h = wo + wi
    with np.errstate(divide="ignore", invalid="ignore"):
        h = h / np.linalg.norm(h, axis=1, keepdims=True)
    ok = (wi[:, 2] > 0) & (wo[:, 2] > 0)
    D = _mf_eval(distr, a, h)
    g1i = _mf_smith_g1(distr, a, wi, h)
    cih = (wi * h).sum(axis=1)
    pdf = np.where(ok & (cih > 0) & ((wo * h).sum(axis=1) > 0), D * g1i / (4.0 * wi[:, 2]), 0.0)
    val = np.where(ok & (D != 0), D * g1i * _mf_smith_g1(distr, a, wo, h) / (4.0 * wi[:, 2]), 0.0)
    return np.nan_to_num(val), np.nan_to_num(pdf), cih


def _conductor_samples(em, normals, wi_world, distr, alpha, seed, spp, lam):
    """Per sample of direct_conductor, from the PCG32Sampler streams: u_em = next_2d, sample_1 =
    next_1d (unused by the conductor), u_bsdf = next_2d (path.cpp:216-234)."""
    normals = np.asarray(normals, dtype=np.float32)
    n = normals.shape[0]
    rng = Pcg32(seed, n)
    s, t = _coordinate_system(normals)
    wv = np.asarray(wi_world, dtype=np.float32)
    wi = np.stack([(wv * s).sum(1), (wv * t).sum(1), (wv * normals).sum(1)], axis=1).astype(np.float64)
    au, av = _auv(alpha)
    a = (max(au, 1e-4), max(av, 1e-4))   # MicrofacetDistribution::configure, microfacet.h:424-428
    for _ in range(spp):
        u0, u1 = rng.next_float(), rng.next_float()
        rng.next_float()
        u2, u3 = rng.next_float(), rng.next_float()
        r = em.sample_direction(np.stack([u0, u1], axis=1), wavelengths=lam)
        d = r["d"].astype(np.float64)
        wo = np.stack([(d * s).sum(1), (d * t).sum(1), (d * normals).sum(1)], axis=1)
        dg, bpdf, cih = _conductor_eval_pdf(distr, a, wi, wo)
        em_ok = (r["pdf"] != 0) & (dg != 0)
        m, mpdf = _mf_sample(distr, a, np.where(wi[:, 2:] > 0, wi, np.array([0.0, 0.0, 1.0])), np.stack([u2, u3], 1))
        dwm = (wi * m).sum(1)
        ro = 2.0 * dwm[:, None] * m - wi
        with np.errstate(divide="ignore", invalid="ignore"):
            pb = mpdf / (4.0 * (ro * m).sum(1))
        b_ok = (wi[:, 2] > 0) & (pb != 0) & np.isfinite(pb) & (ro[:, 2] > 0)
        g1 = _mf_smith_g1(distr, a, ro, m)
        dw = (s * ro[:, :1] + t * ro[:, 1:2] + normals * ro[:, 2:3]).astype(np.float32)
        yield r, dg, bpdf, cih, em_ok, dw, pb, b_ok, g1, dwm


def direct_conductor(em, normals, wi_world, alpha=0.1, distribution="beckmann", eta=0.0, k=1.0, seed=0, spp=1,
                     wavelengths=None, vis=None):
    """Sun-and-sky light a rough conductor reflects towards wi (one vertex of
    src/integrators/path.cpp:176-250 with src/bsdfs/roughconductor.cpp; alpha = a float or
    (alpha_u, alpha_v)): emitter sampling
    (f cos x weight x MIS) + visible-normal BSDF sampling (F G1(wo) x eval x MIS), power
    heuristic, spp samples.  em: an Oracle; eta / k: 1 or 3 values (spectral: the first).
    vis: None or (spp, n) uint8 tracer verdicts.  Returns (C, n) fp64."""
    normals = np.asarray(normals, dtype=np.float32)
    n = normals.shape[0]
    c = wavelengths.shape[0] if em.spectral else 3
    lam = None if not em.spectral else np.asarray(wavelengths, dtype=np.float32)
    e3 = np.broadcast_to(np.asarray(eta, np.float64), (3,))
    k3 = np.broadcast_to(np.asarray(k, np.float64), (3,))
    etas = np.full(c, e3[0]) if em.spectral else e3
    ks = np.full(c, k3[0]) if em.spectral else k3
    acc = np.zeros((c, n), dtype=np.float64)
    for j, (r, dg, bpdf, cih, em_ok, dw, pb, b_ok, g1, dwm) in enumerate(
            _conductor_samples(em, normals, wi_world, distribution.lower(), alpha, seed, spp, lam)):
        v = np.full(n, 3, np.uint8) if vis is None else np.asarray(vis[j], dtype=np.uint8)
        ok = em_ok & ((v & 1) != 0)
        mis = np.where(ok, _mis_power(r["pdf"], bpdf), 0.0)
        for ch in range(c):
            F = _fresnel_conductor(cih, etas[ch], ks[ch])
            acc[ch] += np.where(ok, F * dg * r["weight"][:, ch] * mis, 0.0)
        esc = b_ok & ((v & 2) != 0)
        dws = np.where(esc[:, None], dw, np.array([0, 0, 1], np.float32))
        mis_b = np.where(esc, _mis_power(pb, em.pdf_direction(dws)), 0.0)
        e = em.eval(-dws, lam) if em.spectral else em.eval(-dws).T
        for ch in range(c):
            F = _fresnel_conductor(dwm, etas[ch], ks[ch])
            acc[ch] += np.where(esc, F * g1 * e[ch] * mis_b, 0.0)
    return acc / spp


def direct_conductor_rays(em, normals, wi_world, alpha=0.1, distribution="beckmann", seed=0, spp=1, eta=None,
                          k=None):
    """The rays a tracer tests for direct_conductor: emitter-sample and BSDF directions, each
    (spp, n, 3) fp32, zero where no ray is needed; with eta / k also the BSDF samples' weights
    F(wi.m) G1(wo, m) (roughconductor.cpp sample()), (C, spp, n) fp64 with C = 3 (RGB) or 1."""
    em_d, bs_d, bw = [], [], []
    if eta is not None:
        e3 = np.broadcast_to(np.asarray(eta, np.float64), (3,))[: 1 if em.spectral else 3]
        k3 = np.broadcast_to(np.asarray(k, np.float64), (3,))[: 1 if em.spectral else 3]
    lam = None if not em.spectral else np.full((1, len(normals)), 500.0, np.float32)
    for r, dg, bpdf, cih, em_ok, dw, pb, b_ok, g1, dwm in _conductor_samples(
            em, normals, wi_world, distribution.lower(), alpha, seed, spp, lam):
        em_d.append(np.where(em_ok[:, None], r["d"], 0.0).astype(np.float32))
        bs_d.append(np.where(b_ok[:, None], dw, 0.0).astype(np.float32))
        if eta is not None:
            bw.append(np.stack([np.where(b_ok, _fresnel_conductor(dwm, e, kk) * g1, 0.0) for e, kk in zip(e3, k3)]))
    if eta is None:
        return np.stack(em_d), np.stack(bs_d)
    return np.stack(em_d), np.stack(bs_d), np.stack(bw, axis=1)
