"""The gradients of the sequence irradiance without a GPU (host-only sequences): the ABI
additions, the refusals of sunsky_sequence_irradiance_vjp in the order the header gives them, the
life cycle of the preparation (sticky across prepare_irradiance, dropped by update), the shape of
the reduction as the Python side restates it, and the argument validation of the Python layer."""
import ctypes as C

import numpy as np
import pytest
import torch

import sunsky_amd as ss
from sunsky_amd import _capi
from sequence_cases import LAMBDAS, TURBIDITY, WEIGHTS, base_dict, frame_dirs

NEW_SYMBOLS = ["sunsky_sequence_prepare_irradiance_grad", "sunsky_sequence_irradiance_vjp"]
VARIANTS = ["rgb", "spectral"]


def test_library_exports_the_irradiance_gradient_abi():
    L = C.CDLL(ss.LIB_PATH)
    declared = ss.declared_functions()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in _capi._SIGS, name
    assert ss.lib().sunsky_abi_version() == 7
    for name in ("prepare_irradiance_grad", "irradiance_vjp"):
        assert hasattr(ss.SunskySequence, name)
    assert "sequence_irradiance" in ss.__all__ and callable(ss.sequence_irradiance)


def host_sequence(variant):
    parent = ss.SunskyEmitter(base_dict(), variant=variant, device="host")
    return ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)


@pytest.mark.parametrize("variant", VARIANTS)
def test_refusals_and_lifecycle(variant):
    seq = host_sequence(variant)
    lam = LAMBDAS if variant == "spectral" else None
    L = ss.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    v3, out3, none3 = _capi.Vec3In(p, p, p), _capi.Vec3Out(p, p, p), _capi.Vec3Out(None, None, None)

    def vjp(n=4, d=p, gn=out3, gw=p):
        return L.sunsky_sequence_irradiance_vjp(seq._h, v3, None, n, d, n, gn, gw, None)

    nrm, d4 = np.zeros((3, 4), np.float32), np.zeros((5 if lam else 3, 4), np.float32)
    # before either preparation: the tables are named first
    assert seq.irradiance_args is None and not seq.irradiance_grad_prepared
    assert vjp() == 1 and b"sunsky_sequence_prepare_irradiance first" in L.sunsky_last_error()
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.irradiance_vjp(nrm, d4)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.prepare_irradiance_grad()
    assert not seq.irradiance_grad_prepared
    # tables, but no gradient preparation
    seq.prepare_irradiance(8, 16, wavelengths=lam)
    assert seq.irradiance_args == (8, 16, None if lam is None else [float(x) for x in lam])
    assert vjp() == 1 and b"sunsky_sequence_prepare_irradiance_grad first" in L.sunsky_last_error()
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance_grad first"):
        seq.irradiance_vjp(nrm, d4)
    # prepared (a state change on a host-only sequence): the launch itself is refused, no pointer is read
    seq.prepare_irradiance_grad()
    assert seq.irradiance_grad_prepared
    assert vjp() == 1 and b"host-only sequence" in L.sunsky_last_error()
    with pytest.raises(ValueError, match="host-only"):
        seq.irradiance_vjp(nrm, d4)
    # arguments: n == 0 succeeds, d_out is required, either output may be NULL, grad_normal all or nothing
    assert L.sunsky_sequence_irradiance_vjp(seq._h, _capi.Vec3In(None, None, None), None, 0, None, 0, none3, None, None) == 0
    assert vjp(d=None) == 1 and b"d_out" in L.sunsky_last_error()
    assert L.sunsky_sequence_irradiance_vjp(seq._h, _capi.Vec3In(None, p, p), None, 4, p, 4, out3, p, None) == 1
    assert vjp(gn=_capi.Vec3Out(p, None, p)) == 1 and b"grad_normal" in L.sunsky_last_error()
    assert vjp(gn=none3) == 1 and b"host-only sequence" in L.sunsky_last_error()
    assert vjp(gw=None) == 1 and b"host-only sequence" in L.sunsky_last_error()
    assert vjp(n=1 << 32) == 1 and b"2^32" in L.sunsky_last_error()
    assert L.sunsky_sequence_irradiance_vjp(None, v3, None, 4, p, 4, out3, p, None) == 1
    assert L.sunsky_sequence_prepare_irradiance_grad(None) == 1
    # sticky: new tables restage it
    seq.prepare_irradiance(16, 32, wavelengths=lam)
    assert vjp() == 1 and b"host-only sequence" in L.sunsky_last_error()
    # update drops it together with the tables
    seq.update(weights=[1.0] * 5)
    assert vjp() == 1 and b"sunsky_sequence_prepare_irradiance first" in L.sunsky_last_error()
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.prepare_irradiance_grad()
    # and prepare_irradiance alone brings both back
    seq.prepare_irradiance(8, 16, wavelengths=lam)
    assert vjp() == 1 and b"host-only sequence" in L.sunsky_last_error()
    # the table read-back takes no new ids
    assert L.sunsky_sequence_get_irradiance_table(seq._h, 2, None, 0, None) == 1


def test_a_sequence_that_never_asked_for_gradients_does_not_get_them():
    seq = host_sequence("rgb")
    seq.prepare_irradiance(8, 16)
    seq.update(weights=[1.0] * 5)
    seq.prepare_irradiance(8, 16)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance_grad first"):
        seq.irradiance_vjp(np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32))


def test_reduction_shape_is_the_headers():
    """slices_wanted = ceil(n / 1024) <= min(64, floor(bound / (P (Q + K)))) (at least 1); the
    length is ceil(n / slices_wanted) rounded up to 256; the slices in use are ceil(n / length)."""
    shape = _capi.seq_irr_grad_shape
    assert shape(1, 3, 512, 5) == (1, 256)
    assert shape(1024, 3, 512, 5) == (1, 1024)
    assert shape(1025, 3, 512, 5) == (2, 768)
    assert shape(4099, 3, 512, 5) == (5, 1024)
    assert shape(4096, 3, 512, 5) == (4, 1024)
    assert shape(1 << 20, 3, 64 * 256, 24) == (64, 16384)
    assert shape(1 << 20, 32, 64 * 256, 24) == (7, 150016)          # 2^22 / (32 x 16408) = 7.99: 7 rows
    assert shape(4099, 3, 512, 5, 3200) == (2, 2304)
    assert shape(4099, 5, 512, 5, 3200) == (1, 4352)
    assert shape(4099, 32, 1 << 20, 5, 1 << 22) == (1, 4352)         # one row is more than the bound
    for n in (1, 255, 256, 257, 4099, 70001, (1 << 32) - 256):
        for cap in (1, 3200, 1 << 22):
            s, length = shape(n, 3, 512, 5, cap)
            assert length % 256 == 0 and (s - 1) * length < n <= s * length
            assert s <= max(1, min(64, cap // (3 * 517)))


@pytest.mark.parametrize("variant", VARIANTS)
def test_python_argument_validation(variant):
    seq = host_sequence(variant)
    with pytest.raises(ValueError, match="shape \\(3, n\\)"):
        ss.sequence_irradiance(seq, torch.zeros(4, 3))
    with pytest.raises(ValueError, match="shape \\(3, n\\)"):
        ss.sequence_irradiance(seq, np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="weights must be a float32 tensor"):
        ss.sequence_irradiance(seq, torch.zeros(3, 4), weights=[1.0] * 5)
    with pytest.raises(ValueError, match="weights must be a float32 tensor"):
        ss.sequence_irradiance(seq, torch.zeros(3, 4), weights=torch.ones(5, dtype=torch.float64))
    # with weights the forward prepares again with the remembered arguments: there must be some
    with pytest.raises(ValueError, match="prepare_irradiance"):
        ss.sequence_irradiance(seq, torch.zeros(3, 4), weights=torch.ones(5))
    # a host-only sequence refuses the forward after the update and the preparation
    seq.prepare_irradiance(8, 16, wavelengths=LAMBDAS if variant == "spectral" else None)
    with pytest.raises(ValueError, match="host-only"):
        ss.sequence_irradiance(seq, torch.zeros(3, 4), weights=torch.full((5,), 2.0))
    assert seq.frame(0)["weight"] == 2.0 and seq.irradiance_info()["n_z"] == 8
    with pytest.raises(ValueError, match="must have 5 values"):
        ss.sequence_irradiance(seq, torch.zeros(3, 4), weights=torch.ones(4))
