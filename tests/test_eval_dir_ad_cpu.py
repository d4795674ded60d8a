"""eval_jvp_dir / eval_vjp_dir (d eval / d wi) without a GPU: the symbols and their bindings,
the C ABI's argument validation on host-only emitters (mirrors test_jvp_argument_validation_host),
and the Python wrappers' shape / dtype checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sunsky_amd as ss
from helpers import angles_dict

SCENE = angles_dict(3.4, 0.6, math.pi / 2 - math.radians(40), 0.3, 1.0, 1.0)


def _planes(rows, n):
    """Host memory standing in for device planes: a host-only emitter validates its arguments
    and fails before anything reads them."""
    a = np.zeros((rows, max(n, 1)), np.float32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _v3(a, cls):
    p = [a[i].ctypes.data_as(ctypes.c_void_p) for i in range(3)]
    return cls(*p)


def test_symbols_are_exported_and_bound():
    lib = ss.lib()
    for name in ("sunsky_eval_jvp_dir", "sunsky_eval_vjp_dir"):
        assert name in ss._capi._SIGS
        f = getattr(lib, name)
        assert f.argtypes == ss._capi._SIGS[name][1] and f.restype is ctypes.c_int
    assert lib.sunsky_abi_version() == 7   # additive: the version stays


def test_eval_wi_is_exported():
    assert callable(ss.eval_wi) and "eval_wi" in ss.__all__


def test_dir_ad_argument_validation_host():
    lib = ss.lib()
    V3, V3o = ss._capi.Vec3In, ss._capi.Vec3Out
    none_in, none_out = V3(None, None, None), V3o(None, None, None)
    n = 8
    w, _ = _planes(3, n)
    dw, _ = _planes(3, n)
    o, op = _planes(4, n)
    do, dop = _planes(4, n)
    g, _ = _planes(3, n)
    lam, lp = _planes(4, n)
    wi, dwi, gout = _v3(w, V3), _v3(dw, V3), _v3(g, V3o)
    rgb = ss.SunskyEmitter(SCENE, "rgb", device="host")
    spec = ss.SunskyEmitter(SCENE, "spectral", device="host")

    def jvp(e, wi_, dwi_, lam_, nl, ls, n_, o_, do_, os_):
        return lib.sunsky_eval_jvp_dir(e._h if e else None, wi_, dwi_, lam_, nl, ls, None, n_, o_, do_, os_, None)

    def vjp(e, wi_, lam_, nl, ls, n_, do_, os_, g_):
        return lib.sunsky_eval_vjp_dir(e._h if e else None, wi_, lam_, nl, ls, None, n_, do_, os_, g_, None)

    # null emitter
    assert jvp(None, wi, dwi, None, 0, 0, n, op, dop, n) != 0
    assert b"null emitter" in lib.sunsky_last_error()
    assert vjp(None, wi, None, 0, 0, n, dop, n, gout) != 0
    # n = 0 succeeds and touches nothing: null planes are allowed; an RGB emitter ignores wavelengths
    assert jvp(rgb, none_in, none_in, None, 0, 0, 0, None, None, 0) == 0
    assert vjp(rgb, none_in, None, 0, 0, 0, None, 0, none_out) == 0
    assert jvp(rgb, none_in, none_in, None, 99, 0, 0, None, None, 0) == 0
    # a spectral emitter needs 1..16 wavelength planes, even at n = 0
    assert jvp(spec, none_in, none_in, None, 4, 0, 0, None, None, 0) == 0
    assert vjp(spec, none_in, None, 4, 0, 0, None, 0, none_out) == 0
    for bad in (0, -1, 17):
        assert jvp(spec, none_in, none_in, None, bad, 0, 0, None, None, 0) != 0
        assert b"wavelength planes" in lib.sunsky_last_error()
        assert vjp(spec, none_in, None, bad, 0, 0, None, 0, none_out) != 0
        assert b"wavelength planes" in lib.sunsky_last_error()
    # null planes at n > 0
    assert jvp(rgb, none_in, dwi, None, 0, 0, n, op, dop, n) != 0
    assert b"null" in lib.sunsky_last_error()
    assert jvp(rgb, wi, none_in, None, 0, 0, n, op, dop, n) != 0
    assert jvp(rgb, wi, dwi, None, 0, 0, n, None, dop, n) != 0
    assert jvp(rgb, wi, dwi, None, 0, 0, n, op, None, n) != 0
    assert vjp(rgb, none_in, None, 0, 0, n, dop, n, gout) != 0
    assert vjp(rgb, wi, None, 0, 0, n, None, n, gout) != 0
    assert vjp(rgb, wi, None, 0, 0, n, dop, n, none_out) != 0
    assert b"null" in lib.sunsky_last_error()
    assert jvp(spec, wi, dwi, None, 4, n, n, op, dop, n) != 0    # spectral, n > 0: null wavelengths
    assert vjp(spec, wi, None, 4, n, n, dop, n, gout) != 0
    # strides
    assert jvp(rgb, wi, dwi, None, 0, 0, n, op, dop, n - 1) != 0
    assert b"out_stride" in lib.sunsky_last_error()
    assert vjp(rgb, wi, None, 0, 0, n, dop, n - 1, gout) != 0
    assert b"out_stride" in lib.sunsky_last_error()
    assert jvp(spec, wi, dwi, lp, 4, n - 1, n, op, dop, n) != 0
    assert b"wl_stride" in lib.sunsky_last_error()
    assert vjp(spec, wi, lp, 4, n - 1, n, dop, n, gout) != 0
    assert b"wl_stride" in lib.sunsky_last_error()
    # valid arguments: a host-only emitter then fails like the other batch calls, reading nothing
    for e, lam_, nl, ls in ((rgb, None, 0, 0), (spec, lp, 4, n)):
        want = lib.sunsky_eval(e._h, wi, lam_, nl, ls, None, n, op, n, None)
        text = lib.sunsky_last_error()
        assert want != 0
        assert jvp(e, wi, dwi, lam_, nl, ls, n, op, dop, n) == want
        assert lib.sunsky_last_error() == text
        assert vjp(e, wi, lam_, nl, ls, n, dop, n, gout) == want
        assert lib.sunsky_last_error() == text
    assert not o.any() and not do.any() and not g.any()


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_python_wrappers_reject_wrong_shapes_and_dtypes(variant):
    em = ss.SunskyEmitter(SCENE, variant, device="host")
    n, k = 5, (4 if variant == "spectral" else 3)
    lam = torch.full((4, n), 550.0) if variant == "spectral" else None
    si = ss.SurfaceInteraction3f(wi=torch.zeros(3, n), wavelengths=lam)
    ok_d, ok_c = torch.zeros(3, n), torch.zeros(k, n)
    for bad in (torch.zeros(3, n + 1), torch.zeros(n, 3), torch.zeros(2, n), torch.zeros(3 * n),
                torch.zeros(3, n, dtype=torch.float64), torch.zeros(3, n, dtype=torch.int32)):
        with pytest.raises(ValueError):
            em.eval_jvp_dir(si, bad)
    for bad in (torch.zeros(k, n + 1), torch.zeros(k + 1, n), torch.zeros(n, k), torch.zeros(k * n),
                torch.zeros(k, n, dtype=torch.float64), torch.zeros(k, n, dtype=torch.float16)):
        with pytest.raises(ValueError):
            em.eval_vjp_dir(si, bad)
    for bad in (torch.zeros(3, n + 1), torch.zeros(n, 3), torch.zeros(3, n, dtype=torch.float64),
                torch.zeros(3, 2 * n)[:, ::2], np.zeros((3, n), np.float32)):
        with pytest.raises(ValueError):
            em.eval_vjp_dir(si, ok_c, out=bad)
    with pytest.raises(ValueError):
        em.eval_jvp_dir(ss.SurfaceInteraction3f(wi=torch.zeros(2, n), wavelengths=lam), ok_d)
    with pytest.raises(ValueError):
        em.eval_vjp_dir(si, ok_c, active=torch.ones(n + 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        em.eval_jvp_dir(si, ok_d, active=torch.ones(n - 1, dtype=torch.bool))
    if variant == "spectral":
        with pytest.raises(ValueError):
            em.eval_jvp_dir(ss.SurfaceInteraction3f(wi=torch.zeros(3, n)), ok_d)
        with pytest.raises(ValueError):
            em.eval_vjp_dir(ss.SurfaceInteraction3f(wi=torch.zeros(3, n), wavelengths=torch.zeros(17, n)), ok_c)
    for bad in (torch.zeros(3, n, dtype=torch.float64), torch.zeros(n, 3), np.zeros((3, n), np.float32)):
        with pytest.raises(ValueError):
            ss.eval_wi(em, bad, lam)
