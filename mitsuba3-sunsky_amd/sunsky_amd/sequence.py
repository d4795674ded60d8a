"""Weighted frame sequences over one emitter (sunsky_sequence_*, include/sunsky_amd.h):
out = sum_k w_k eval_k(wi) for K sun directions / turbidities in one launch -- a time-lapse,
a cumulative-sky map, a time-averaged sky.  The sequence is a snapshot of the emitter at
creation; it keeps no reference to it.
"""
import ctypes as C
import datetime
import math

import numpy as np
import torch

from . import _capi
from ._capi import Vec3In, check, lib
from .emitter import SunskyEmitter, _PRECISION, _fa, _ptr


def sun_coordinates(year, month, day, hour, minute=0.0, second=0.0, latitude=35.6894, longitude=139.6917,
                    timezone=9.0):
    """compute_sun_coordinates (sunsky.h:284-374) in fp32, as the emitter's time/location mode
    evaluates it: the unit sun direction in the emitter's local frame (z up)."""
    out = (C.c_float * 3)()
    check(lib().sunsky_sun_coordinates(int(year), int(month), int(day), float(hour), float(minute), float(second),
                                       float(latitude), float(longitude), float(timezone), out))
    return np.array(out, dtype=np.float32)


def horizon_from_elevation(degrees):
    """sin of horizon elevation angles in degrees as fp32, the unit of SunskySequence.irradiance's
    `horizon`: a tensor stays a tensor (on its device), anything else becomes a numpy array."""
    if isinstance(degrees, torch.Tensor):
        return torch.sin(torch.deg2rad(degrees.to(torch.float64))).to(torch.float32)
    return np.sin(np.deg2rad(np.asarray(degrees, dtype=np.float64))).astype(np.float32)


def _time_fields(t):
    if isinstance(t, datetime.datetime):
        return t.year, t.month, t.day, float(t.hour), float(t.minute), t.second + t.microsecond * 1e-6
    f = tuple(t)
    if not 4 <= len(f) <= 6:
        raise ValueError("a time is a datetime or (year, month, day, hour[, minute[, second]])")
    return f + (0.0,) * (6 - len(f))


class SunskySequence:
    """K frames (sun direction, turbidity, weight) over a snapshot of `em`.

    sun_directions -- (K, 3) world-space directions (normalised like the emitter's sun_direction)
    turbidity      -- K values in [1, 10], a scalar, or None (the emitter's)
    weights        -- K finite values >= 0, or None (1)
    """

    def __init__(self, em, sun_directions, turbidity=None, weights=None):
        self._h = None
        self.grad_prepared = False
        self.irradiance_args = None            # (n_z, n_phi, wavelengths) of the last prepare_irradiance
        self.irradiance_grad_prepared = False
        d = self._dirs(sun_directions)
        k = d.shape[0]
        t, w = self._per_frame(turbidity, k, "turbidity"), self._per_frame(weights, k, "weights")
        self.device = em.device
        self.variant, self.is_spectral = em.variant, em.is_spectral
        h = C.c_void_p()
        check(lib().sunsky_sequence_create(em._h, k, _fa(d.reshape(-1).tolist()), t, w, C.byref(h)))
        self._h = h

    @staticmethod
    def _dirs(v):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        d = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError("sun_directions must have shape (K, 3)")
        return d

    @staticmethod
    def _per_frame(v, k, name):
        if v is None:
            return None
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        a = np.asarray(v, dtype=np.float32)
        if a.ndim == 0:
            a = np.full(k, a, dtype=np.float32)
        if a.shape != (k,):
            raise ValueError(f"{name} must have {k} values (one per frame), got shape {a.shape}")
        return _fa(a.tolist())

    @classmethod
    def from_times(cls, em, times, latitude=35.6894, longitude=139.6917, timezone=9.0, turbidity=None, weights=None):
        """Frames at the sun positions of `times` (datetimes or (year, month, day, hour[, minute[,
        second]]) tuples) at one place, through sunsky_sun_coordinates and the emitter's to_world.
        Night hours are valid frames (a sun below the horizon contributes no sky)."""
        m = np.asarray(em.get_param("to_world"), dtype=np.float32)[:3, :3]
        dirs = [m @ sun_coordinates(*_time_fields(t), latitude=latitude, longitude=longitude, timezone=timezone)
                for t in times]
        return cls(em, np.asarray(dirs, dtype=np.float32).reshape(-1, 3), turbidity, weights)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            try:
                lib().sunsky_sequence_destroy(h)
            except Exception:   # interpreter shutdown: the library may already be gone
                pass

    def __len__(self):
        return self.info()["count"]

    def info(self):
        d = _capi.SequenceDesc()
        check(lib().sunsky_sequence_info(self._h, C.byref(d)))
        return {"count": d.count, "variant": d.variant, "nb_channels": d.nb_channels,
                "precision": "fast" if d.precision == _capi.PRECISION_FAST else "reference", "device": d.device}

    def set_precision(self, precision):
        check(lib().sunsky_sequence_set_precision(self._h, _PRECISION[precision]))

    def frame(self, k):
        """Frame k as staged: local sun direction, weight, turbidity, (nch, 9) sky coefficients and
        nch sky radiances (the layout of table("sky_params") / table("sky_radiance"))."""
        nch = self.info()["nb_channels"]
        sd, w, t = (C.c_float * 3)(), C.c_float(), C.c_float()
        sp, sr = (C.c_float * (nch * 9))(), (C.c_float * nch)()
        check(lib().sunsky_sequence_get_frame(self._h, int(k), sd, C.byref(w), C.byref(t), sp, sr))
        return {"sun_dir_local": np.array(sd, dtype=np.float32), "weight": w.value, "turbidity": t.value,
                "sky_params": np.array(sp, dtype=np.float32).reshape(nch, 9),
                "sky_radiance": np.array(sr, dtype=np.float32)}

    def _stream(self):
        if self.device is None:
            return C.c_void_p()
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _lambda(self, wavelengths, what):
        if not self.is_spectral:
            if wavelengths is not None:
                raise ValueError(f"an RGB {what} takes no wavelengths")
            return 3, None, 0
        if wavelengths is None:
            raise ValueError(f"a spectral {what} needs a wavelength list")
        lam = [float(x) for x in np.atleast_1d(np.asarray(wavelengths, dtype=np.float32))]
        return len(lam), _fa(lam), len(lam)

    def eval(self, si_or_wi, wavelengths=None, active=None, out=None):
        """sum_k w_k eval_k(si) -> (3, n) RGB, or (m, n) for one wavelength list broadcast to every
        ray (spectral).  si_or_wi: a SurfaceInteraction3f or a (3, n) wi tensor."""
        if self.device is None:
            raise ValueError("host-only sequence (over a host-only emitter) cannot launch kernels")
        wi = getattr(si_or_wi, "wi", si_or_wi)
        wi, vin = SunskyEmitter._vec_in(self, wi)
        n = wi.shape[1]
        k, lam_p, m = self._lambda(wavelengths, "sequence eval")
        out = SunskyEmitter._out(self, out, (k, n), row_stride_ok=True)
        mask = SunskyEmitter._mask(self, active, n)
        check(lib().sunsky_sequence_eval(self._h, vin, lam_p, m, _ptr(mask), n, _ptr(out), out.stride(0), self._stream()))
        return out

    def bake_latlong(self, width, height, theta=(0.0, math.pi), phi=(0.0, 2 * math.pi), wavelengths=None, out=None):
        """Lat-long map of the weighted sum (sunsky_sequence_bake_latlong): (C, height, width), the
        grid of SunskyEmitter.bake_latlong."""
        if self.device is None:
            raise ValueError("host-only sequence (over a host-only emitter) cannot launch kernels")
        k, lam_p, m = self._lambda(wavelengths, "sequence bake")
        out = SunskyEmitter._out(self, out, (k, height, width))
        check(lib().sunsky_sequence_bake_latlong(self._h, width, height, float(theta[0]), float(theta[1]),
                                                 float(phi[0]), float(phi[1]), lam_p, m, _ptr(out), height * width,
                                                 self._stream()))
        return out

    # ------------------------------------------------------------ importance sampling
    def prepare_sampling(self, n_z=64, n_phi=256):
        """Builds the sampling distribution (sunsky_sequence_prepare_sampling): an n_z x n_phi
        equal-solid-angle table of the cumulative sky's luminance and one cone per frame.
        Host-synchronous; a second call replaces the tables.  Works on host-only sequences."""
        check(lib().sunsky_sequence_prepare_sampling(self._h, int(n_z), int(n_phi)))

    def sampling_info(self):
        d = _capi.SequenceSamplingDesc()
        check(lib().sunsky_sequence_sampling_info(self._h, C.byref(d)))
        return {"n_z": d.n_z, "n_phi": d.n_phi, "w_sky": d.w_sky, "sky_mass": d.sky_mass, "sun_mass": d.sun_mass}

    def sampling_table(self, name):
        """One table of the distribution as fp32: "sky" (n_z, n_phi), "row_cdf" (n_z,), "cell_cdf"
        (n_z, n_phi), "q", "frame_cdf", "B" (count,)."""
        tid = _capi.SEQUENCE_TABLES[name]
        cnt = C.c_size_t()
        check(lib().sunsky_sequence_get_sampling_table(self._h, tid, None, 0, C.byref(cnt)))
        buf = (C.c_float * cnt.value)()
        check(lib().sunsky_sequence_get_sampling_table(self._h, tid, buf, cnt.value, C.byref(cnt)))
        a = np.array(buf, dtype=np.float32)
        if name in ("sky", "cell_cdf"):
            i = self.sampling_info()
            a = a.reshape(i["n_z"], i["n_phi"])
        return a

    def sample_direction(self, it, sample, wavelengths=None, active=None):
        """(DirectionSample3f, weight) in SunskyEmitter.sample_direction's shape: ds.d, ds.pdf,
        ds.p / ds.dist from it.p (None = origin) and the snapshot's bounding sphere, and
        weight = sum_k w_k eval_k(-ds.d) / ds.pdf as (3, n) RGB or (m, n) for one wavelength list."""
        from .records import DirectionSample3f
        if self.device is None:
            self.sampling_info()   # an unprepared sequence says so first
            raise ValueError("host-only sequence (over a host-only emitter) cannot launch kernels")
        sample = self._f32(sample)
        if sample.dim() != 2 or sample.shape[0] != 2:
            raise ValueError("sample is a (2, n) tensor")
        n = sample.shape[1]
        k, lam_p, m = self._lambda(wavelengths, "sequence sample_direction")
        mask = SunskyEmitter._mask(self, active, n)
        p = getattr(it, "p", None) if it is not None else None
        if p is not None:
            p, pin = SunskyEmitter._vec_in(self, p, n, "it.p")
        else:
            pin = Vec3In(None, None, None)
        d = torch.empty((3, n), dtype=torch.float32, device=self.device)
        pos = torch.empty((3, n), dtype=torch.float32, device=self.device)
        pdf = torch.empty(n, dtype=torch.float32, device=self.device)
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        w = torch.empty((k, n), dtype=torch.float32, device=self.device)
        check(lib().sunsky_sequence_sample_direction(
            self._h, _ptr(sample[0]), _ptr(sample[1]), pin, lam_p, m, _ptr(mask), n,
            _capi.Vec3Out(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr()), _ptr(pdf), _ptr(dist),
            _capi.Vec3Out(pos[0].data_ptr(), pos[1].data_ptr(), pos[2].data_ptr()), _ptr(w), n, self._stream()))
        ds = DirectionSample3f(p=pos, n=-d, uv=sample, time=getattr(it, "time", None), pdf=pdf, delta=False, d=d,
                               dist=dist, emitter=self)
        return ds, w

    def pdf_direction(self, it, ds, active=None):
        """The sampling density of ds.d (n,): what sample_direction stores in ds.pdf."""
        if self.device is None:
            self.sampling_info()
            raise ValueError("host-only sequence (over a host-only emitter) cannot launch kernels")
        d, vin = SunskyEmitter._vec_in(self, getattr(ds, "d", ds))
        n = d.shape[1]
        mask = SunskyEmitter._mask(self, active, n)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        check(lib().sunsky_sequence_pdf_direction(self._h, vin, _ptr(mask), n, _ptr(out), self._stream()))
        return out

    # ------------------------------------------------------------ irradiance on receivers
    def prepare_irradiance(self, n_z=64, n_phi=256, wavelengths=None):
        """Builds the irradiance tables (sunsky_sequence_prepare_irradiance): the cumulative sky
        per plane over an n_z x n_phi equal-solid-angle grid and one disc flux per frame and plane.
        Planes: RGB, or one per entry of `wavelengths` (spectral, at most 32).  Host-synchronous;
        a second call replaces the tables; independent of prepare_sampling.  Works on host-only
        sequences."""
        _, lam_p, m = self._lambda(wavelengths, "sequence prepare_irradiance")
        check(lib().sunsky_sequence_prepare_irradiance(self._h, int(n_z), int(n_phi), lam_p, m))
        # what sequence_irradiance prepares again with after it has updated the weights
        self.irradiance_args = (int(n_z), int(n_phi), None if lam_p is None else [float(x) for x in lam_p])

    def prepare_irradiance_grad(self):
        """Stages what irradiance_vjp reads beside the tables and allocates its bounded reduction
        workspace (sunsky_sequence_prepare_irradiance_grad).  Needs prepare_irradiance; sticky: a
        later prepare_irradiance restages it, update() drops it with the tables.  Host-synchronous;
        a state change only on host-only sequences."""
        check(lib().sunsky_sequence_prepare_irradiance_grad(self._h))
        self.irradiance_grad_prepared = True

    def irradiance_vjp(self, normals, d_out, active=None, grad=None, horizon=None):
        """Reverse mode of irradiance(): with L = sum(d_out * irradiance(normals)), returns
        {"normals": (3, n) dL/dn, written, "weights": (K,) dL/dw_k, accumulated} as device tensors
        -- those of `grad` (an entry set to None is not computed) or new ones.  E is piecewise
        linear in n (the clamp's derivative is the strict step) and linear in w; every frame gets
        its weight gradient, a zero-weight one included.  Needs prepare_irradiance_grad.
        Deterministic; calls on one sequence share a workspace, so order them across streams.

        horizon: irradiance()'s argument; the gradients are then those of
        irradiance(normals, horizon=horizon) (sunsky_sequence_irradiance_horizon_vjp) and the
        result has a third entry, "horizon": dL/dh, written -- (H, n) for per-receiver profiles
        (a row stride is allowed), the profile's own shape for a shared one (the per-receiver
        columns of an internal (H, n) buffer summed by torch.sum).  In `grad`, a "horizon" entry
        that is None or missing is not computed.  None: the unoccluded call, unchanged."""
        if horizon is None and grad is not None and grad.get("horizon") is not None:
            raise ValueError("grad['horizon'] needs a horizon")
        if self.device is None:
            # the library refuses, and says first which preparation is missing; it reads no pointer
            p = C.cast((C.c_float * 1)(), C.c_void_p)
            none = _capi.Vec3Out(None, None, None)
            if horizon is None:
                check(lib().sunsky_sequence_irradiance_vjp(self._h, Vec3In(p, p, p), None, 1, p, 1, none, None, None))
            else:
                self.irradiance_info()   # an unprepared sequence says so first
                n = int(np.shape(normals)[-1])
                _, sectors, profiles, _ = self._horizon(horizon, n)
                if grad is not None:
                    self._grad_horizon(grad.get("horizon"), tuple(horizon.shape), sectors, n,
                                       self._shared_horizon(tuple(horizon.shape), n))
                check(lib().sunsky_sequence_irradiance_horizon_vjp(self._h, Vec3In(p, p, p), p, sectors, 1, 1, None, 1, p, 1,
                                                                   none, None, None, 1, None))
            raise ValueError("host-only sequence (over a host-only emitter) cannot launch kernels")
        nrm, vin = SunskyEmitter._vec_in(self, normals)
        n = nrm.shape[1]
        planes = self.irradiance_info()["n_planes"]
        if horizon is not None:
            hshape = tuple(horizon.shape) if isinstance(horizon, torch.Tensor) else None
            horizon, sectors, profiles, hstride = self._horizon(horizon, n)
        mask = SunskyEmitter._mask(self, active, n)
        d_out = torch.as_tensor(d_out, dtype=torch.float32, device=self.device)
        if tuple(d_out.shape) != (planes, n):
            raise ValueError(f"d_out must have shape ({planes}, {n})")
        if n > 1 and d_out.stride(1) != 1 or planes > 1 and d_out.stride(0) < n:
            d_out = d_out.contiguous()   # rows must be contiguous; a row stride is passed on as it is
        count = len(self)
        shapes = {"normals": (3, n), "weights": (count,)}
        if grad is None:
            grad = {"normals": torch.empty((3, n), dtype=torch.float32, device=self.device),
                    "weights": torch.zeros(count, dtype=torch.float32, device=self.device)}
            if horizon is not None:
                grad["horizon"] = torch.empty(hshape if self._shared_horizon(hshape, n) else (sectors, n),
                                              dtype=torch.float32, device=self.device)
        for key, shape in shapes.items():
            g = grad.get(key)
            if g is not None and (not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device != self.device
                                  or tuple(g.shape) != shape or not g.is_contiguous()):
                raise ValueError(f"grad['{key}'] must be a contiguous float32 tensor of shape {shape} on {self.device}")
        gn, gw = grad.get("normals"), grad.get("weights")
        gout = _capi.Vec3Out(None, None, None) if gn is None else _capi.Vec3Out(*[gn[i].data_ptr() for i in range(3)])
        if horizon is None:
            check(lib().sunsky_sequence_irradiance_vjp(self._h, vin, _ptr(mask), n, _ptr(d_out), max(d_out.stride(0), n),
                                                       gout, _ptr(gw), self._stream()))
            return grad
        gh = grad.get("horizon")
        shared = self._shared_horizon(hshape, n)
        self._grad_horizon(gh, hshape, sectors, n, shared)
        # one column per receiver, also for a shared profile: its columns are summed below
        buf = None if gh is None else torch.empty((sectors, n), dtype=torch.float32, device=self.device) if shared else gh
        check(lib().sunsky_sequence_irradiance_horizon_vjp(self._h, vin, _ptr(horizon), sectors, profiles, hstride,
                                                           _ptr(mask), n, _ptr(d_out), max(d_out.stride(0), n), gout,
                                                           _ptr(gw), _ptr(buf), 0 if buf is None else max(buf.stride(0), n),
                                                           self._stream()))
        if gh is not None and shared and n:
            gh.copy_(torch.sum(buf, dim=1).reshape(gh.shape))
        grad["horizon"] = gh
        return grad

    @staticmethod
    def _shared_horizon(hshape, n):
        """Whether a horizon of this shape is one profile for all n receivers: (H,) always, (H, 1)
        with more than one receiver.  Decided from the shape given, not from n_profiles (which is 1
        for a single receiver either way)."""
        return len(hshape) == 1 or (hshape[1] == 1 and n > 1)

    def _grad_horizon(self, gh, hshape, sectors, n, shared):
        """A grad["horizon"] entry checked against the profile it belongs to: the profile's own
        shape for a shared one, (H, n) with contiguous rows (a row stride is allowed) otherwise."""
        if gh is None:
            return
        shape = hshape if shared else (sectors, n)
        if (not isinstance(gh, torch.Tensor) or gh.dtype != torch.float32
                or (self.device is not None and gh.device != self.device) or tuple(gh.shape) != shape
                or (shared and not gh.is_contiguous())
                or (not shared and (n > 1 and gh.stride(1) != 1 or sectors > 1 and gh.stride(0) < n))):
            where = "" if self.device is None else f" on {self.device}"
            raise ValueError(f"grad['horizon'] must be a float32 tensor of shape {shape}{where}, its rows contiguous")

    def irradiance_info(self):
        d = _capi.SequenceIrradianceDesc()
        check(lib().sunsky_sequence_irradiance_info(self._h, C.byref(d)))
        return {"n_z": d.n_z, "n_phi": d.n_phi, "n_planes": d.n_planes, "omega": d.omega}

    def irradiance_table(self, name):
        """One irradiance table as fp32: "sky" (P, n_z, n_phi), the cumulative sky R_p at the cell
        centres (not multiplied by omega), or "sun_flux" (P, K), the disc fluxes F_k[p] (not
        multiplied by the weights)."""
        tid = _capi.SEQUENCE_IRRADIANCE_TABLES[name]
        cnt = C.c_size_t()
        check(lib().sunsky_sequence_get_irradiance_table(self._h, tid, None, 0, C.byref(cnt)))
        buf = (C.c_float * cnt.value)()
        check(lib().sunsky_sequence_get_irradiance_table(self._h, tid, buf, cnt.value, C.byref(cnt)))
        a = np.array(buf, dtype=np.float32)
        i = self.irradiance_info()
        return a.reshape(i["n_planes"], i["n_z"], i["n_phi"]) if name == "sky" else a.reshape(i["n_planes"], -1)

    def irradiance_sun_columns(self):
        """The grid column j_k of every frame's sun as int32 (K,): what picks a sun's sector of a
        horizon profile (sunsky_sequence_get_irradiance_sun_columns).  Needs prepare_irradiance."""
        cnt = C.c_size_t()
        check(lib().sunsky_sequence_get_irradiance_sun_columns(self._h, None, 0, C.byref(cnt)))
        buf = (C.c_int * cnt.value)()
        check(lib().sunsky_sequence_get_irradiance_sun_columns(self._h, buf, cnt.value, C.byref(cnt)))
        return np.array(buf, dtype=np.int32)

    def _horizon(self, horizon, n):
        """A horizon argument checked against n receivers and the prepared grid: the tensor the
        library reads, then (H, n_profiles, stride between two sectors' planes)."""
        if not isinstance(horizon, torch.Tensor) or horizon.dtype != torch.float32:
            raise ValueError("horizon must be a float32 tensor of shape (H,), (H, 1) or (H, n)")
        if horizon.dim() not in (1, 2) or horizon.shape[0] < 1 or (horizon.dim() == 2 and horizon.shape[1] not in (1, n)):
            raise ValueError(f"horizon must have shape (H,), (H, 1) or (H, {n}), got {tuple(horizon.shape)}")
        sectors, n_phi = horizon.shape[0], self.irradiance_info()["n_phi"]
        if n_phi % sectors:
            raise ValueError(f"the horizon's {sectors} sectors do not divide the irradiance tables' n_phi = {n_phi}")
        if self.device is not None and horizon.device != self.device:
            raise ValueError(f"horizon must be on {self.device}")
        per_receiver = horizon.dim() == 2 and horizon.shape[1] == n and n > 1
        if per_receiver and (horizon.stride(1) != 1 or sectors > 1 and horizon.stride(0) < n):
            horizon = horizon.contiguous()   # rows must be contiguous; a row stride is passed on as it is
        return horizon, sectors, n if per_receiver else 1, horizon.stride(0)

    def irradiance(self, normals, active=None, out=None, horizon=None):
        """E_p(n) of the cumulative sky and suns on receivers with world-space normals (3, n) ->
        (P, n): the fixed quadrature of sunsky_sequence_irradiance over the prepared tables.
        Needs prepare_irradiance; `out` may have a row stride, as eval's.

        horizon: far shading (sunsky_sequence_irradiance_horizon).  A float32 tensor of
        sin(horizon elevation) per azimuth sector of the emitter's local frame (see
        horizon_from_elevation), (H,) or (H, 1) for one profile shared by all receivers, (H, n)
        for one per receiver; H divides the tables' n_phi.  A sector hides the share of each sky
        cell below its horizon and every sun below it.  None: the unoccluded call, unchanged."""
        if self.device is None:
            self.irradiance_info()   # an unprepared sequence says so first
            if horizon is not None:
                self._horizon(horizon, int(np.shape(normals)[-1]))
            raise ValueError("host-only sequence (over a host-only emitter) cannot launch kernels")
        nrm, vin = SunskyEmitter._vec_in(self, normals)
        n = nrm.shape[1]
        planes = self.irradiance_info()["n_planes"]
        if horizon is not None:
            horizon, sectors, profiles, hstride = self._horizon(horizon, n)
        out = SunskyEmitter._out(self, out, (planes, n), row_stride_ok=True)
        mask = SunskyEmitter._mask(self, active, n)
        if horizon is None:
            check(lib().sunsky_sequence_irradiance(self._h, vin, _ptr(mask), n, _ptr(out), out.stride(0), self._stream()))
        else:
            check(lib().sunsky_sequence_irradiance_horizon(self._h, vin, _ptr(horizon), sectors, profiles, hstride,
                                                           _ptr(mask), n, _ptr(out), out.stride(0), self._stream()))
        return out

    # ------------------------------------------------------------ per-frame irradiance series
    def prepare_irradiance_series(self):
        """Stages every frame's own sky image for irradiance_series
        (sunsky_sequence_prepare_irradiance_series): K x P x n_z x n_phi values computed and kept on
        the device, at most 2^26.  Needs prepare_irradiance; sticky: a later prepare_irradiance
        restages it, update() drops it with the tables.  Host-synchronous; a state change only on
        host-only sequences."""
        check(lib().sunsky_sequence_prepare_irradiance_series(self._h))

    def irradiance_frame_table(self, k):
        """Frame k's own sky table as fp32 (P, n_z, n_phi): sky_{k,p} at the cell centres, not
        weighted and not multiplied by omega -- the "sky" table of a sequence that holds frame k
        alone with weight 1.  Needs prepare_irradiance; works on host-only sequences."""
        cnt = C.c_size_t()
        check(lib().sunsky_sequence_get_irradiance_frame_table(self._h, int(k), None, 0, C.byref(cnt)))
        buf = (C.c_float * cnt.value)()
        check(lib().sunsky_sequence_get_irradiance_frame_table(self._h, int(k), buf, cnt.value, C.byref(cnt)))
        i = self.irradiance_info()
        return np.array(buf, dtype=np.float32).reshape(i["n_planes"], i["n_z"], i["n_phi"])

    def _frames(self, frames):
        """A frames argument as (first, count): None (all), a (first, count) pair or a range of step 1."""
        k = len(self)
        if frames is None:
            return 0, k
        if isinstance(frames, range):
            if frames.step != 1:
                raise ValueError("frames must be None, a (first, count) pair or a range with step 1")
            first, count = (frames.start, len(frames)) if len(frames) else (0, 0)
        else:
            try:
                first, count = frames
                ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (first, count))
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("frames must be None, a (first, count) pair or a range with step 1")
            first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > k:
            raise ValueError(f"frames ({first}, {count}) are not within the sequence's {k} frames")
        return first, count

    def irradiance_series(self, normals, frames=None, active=None, out=None, horizon=None):
        """Every frame's own irradiance on receivers with world-space normals (3, n) ->
        (n_frames, P, n): E^k_p(n) of sunsky_sequence_irradiance_series, bit for bit what
        irradiance() gives for a sequence that holds frame k alone with weight 1.  The weights do
        not enter (the caller integrates); night frames give exact zeros.

        frames: None (all), a (first, count) pair or a range with step 1.  `out` may have a row
        stride, as irradiance's; `horizon` takes irradiance's forms.  Needs prepare_irradiance_series."""
        first, count = self._frames(frames)
        if self.device is None:
            # the library refuses, and says first which preparation is missing; it reads no pointer
            p = C.cast((C.c_float * 1)(), C.c_void_p)
            check(lib().sunsky_sequence_irradiance_series(self._h, Vec3In(p, p, p), None, 0, 0, 0, None, 1, 0, 1, p, 1, None))
            raise ValueError("host-only sequence (over a host-only emitter) cannot launch kernels")
        nrm, vin = SunskyEmitter._vec_in(self, normals)
        n = nrm.shape[1]
        planes = self.irradiance_info()["n_planes"]
        sectors = profiles = hstride = 0
        if horizon is not None:
            horizon, sectors, profiles, hstride = self._horizon(horizon, n)
        shape = (count, planes, n)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != self.device
              or tuple(out.shape) != shape):
            raise ValueError(f"out must be a float32 tensor of shape {shape} on {self.device}")
        row = n
        if count * planes > 1 and n > 0:
            row = out.stride(1) if planes > 1 else out.stride(0)
            if not (out.is_contiguous() or ((n == 1 or out.stride(2) == 1) and row >= n
                                            and (count == 1 or planes == 1 or out.stride(0) == planes * row))):
                raise ValueError("out planes must be contiguous (a row stride is allowed)")
        elif not out.is_contiguous() and n > 1 and out.stride(2) != 1:
            raise ValueError("out planes must be contiguous (a row stride is allowed)")
        mask = SunskyEmitter._mask(self, active, n)
        check(lib().sunsky_sequence_irradiance_series(self._h, vin, _ptr(horizon), sectors, profiles, hstride, _ptr(mask), n,
                                                      first, count, _ptr(out), row, self._stream()))
        return out

    # ------------------------------------------------------------ gradients and updates
    def update(self, sun_directions=None, turbidity=None, weights=None):
        """Replaces the frames in place (sunsky_sequence_update): the same count, None keeps the
        current values, the constructor's validation; a refused update leaves the sequence as it
        was.  Afterwards frame() and eval() are bit for bit those of a new sequence with these
        values.  Host-synchronous; drops the sampling distribution (call prepare_sampling again)
        and restages the gradient records if prepare_grad was called."""
        k = len(self)
        d = None
        if sun_directions is not None:
            d = self._dirs(sun_directions)
            if d.shape[0] != k:
                raise ValueError(f"sun_directions must have shape ({k}, 3): update keeps the frame count")
            d = _fa(d.reshape(-1).tolist())
        check(lib().sunsky_sequence_update(self._h, d, self._per_frame(turbidity, k, "turbidity"),
                                           self._per_frame(weights, k, "weights")))

    def prepare_grad(self):
        """Stages the per-frame gradient records and allocates eval_vjp's workspace
        (sunsky_sequence_prepare_grad).  Host-synchronous; works on host-only sequences."""
        check(lib().sunsky_sequence_prepare_grad(self._h))
        self.grad_prepared = True

    def frame_tangent(self, k):
        """Frame k's gradient record: "dsky_turbidity" and "dsky_elevation" (nch, 10) d{A..I, rad}
        along T and along a unit sun elevation, "dsun_local" (3, 3) [a] = d local sun / d s[a] and
        "deta" (3,) d elevation / d s[a] for world axis a (normalisation and to_world folded in)."""
        nch = self.info()["nb_channels"]
        dt, de = (C.c_float * (nch * 10))(), (C.c_float * (nch * 10))()
        dl, deta = (C.c_float * 9)(), (C.c_float * 3)()
        check(lib().sunsky_sequence_get_frame_tangent(self._h, int(k), dt, de, dl, deta))
        return {"dsky_turbidity": np.array(dt, dtype=np.float32).reshape(nch, 10),
                "dsky_elevation": np.array(de, dtype=np.float32).reshape(nch, 10),
                "dsun_local": np.array(dl, dtype=np.float32).reshape(3, 3), "deta": np.array(deta, dtype=np.float32)}

    def eval_vjp(self, si_or_wi, d_out, wavelengths=None, active=None, grad=None):
        """Reverse mode of eval(): with L = sum(d_out * eval(si)), accumulates dL/dw_k, dL/dT_k and
        dL/ds_k (world space) into {"weights": (K,), "turbidity": (K,), "sun_directions": (K, 3)}
        device tensors -- those of `grad` (an entry set to None is not computed) or new zeros --
        and returns the dict.  Needs prepare_grad.  Reference-precision arithmetic, deterministic;
        calls on one sequence share a workspace, so order them when they come from several streams."""
        if self.device is None:
            self.frame_tangent(0)   # an unprepared sequence says so first
            raise ValueError("host-only sequence (over a host-only emitter) cannot launch kernels")
        wi = getattr(si_or_wi, "wi", si_or_wi)
        wi, vin = SunskyEmitter._vec_in(self, wi)
        n = wi.shape[1]
        k, lam_p, m = self._lambda(wavelengths, "sequence eval_vjp")
        mask = SunskyEmitter._mask(self, active, n)
        if d_out is None:
            d_ptr, stride = None, n
        else:
            d_out = self._f32(d_out)
            if tuple(d_out.shape) != (k, n):
                raise ValueError(f"d_out must have shape ({k}, {n})")
            d_ptr, stride = _ptr(d_out), d_out.stride(0)
        count = len(self)
        shapes = {"weights": (count,), "turbidity": (count,), "sun_directions": (count, 3)}
        if grad is None:
            grad = {key: torch.zeros(shape, dtype=torch.float32, device=self.device) for key, shape in shapes.items()}
        ptrs = []
        for key, shape in shapes.items():
            g = grad.get(key)
            if g is not None and (not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or g.device != self.device
                                  or tuple(g.shape) != shape or not g.is_contiguous()):
                raise ValueError(f"grad['{key}'] must be a contiguous float32 tensor of shape {shape} on {self.device}")
            ptrs.append(_ptr(g))
        check(lib().sunsky_sequence_eval_vjp(self._h, vin, lam_p, m, _ptr(mask), n, d_ptr, stride, *ptrs, self._stream()))
        return grad

    # SunskyEmitter's tensor helpers read only self.device
    _f32 = SunskyEmitter._f32
