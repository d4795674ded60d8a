"""Sequence irradiance under a horizon profile without a GPU (host-only sequences): the ABI
additions, every refusal of sunsky_sequence_irradiance_horizon in the header's order, the suns'
grid columns against numpy, their life cycle, the Python argument checks and
horizon_from_elevation."""
import ctypes as C

import numpy as np
import pytest
import torch

import sunsky_amd as ss
from sunsky_amd import _capi
from sequence_cases import LAMBDAS, TURBIDITY, WEIGHTS, base_dict, frame_dirs, rotation

NEW_SYMBOLS = ["sunsky_sequence_irradiance_horizon", "sunsky_sequence_get_irradiance_sun_columns"]
VARIANTS = ["rgb", "spectral"]


def lam_of(variant):
    return LAMBDAS if variant == "spectral" else None


def host_sequence(variant, dirs=None, turb=TURBIDITY, wts=WEIGHTS, **kw):
    parent = ss.SunskyEmitter(base_dict(**kw), variant=variant, device="host")
    return ss.SunskySequence(parent, frame_dirs(kw.get("to_world")) if dirs is None else dirs, turb, wts)


def test_library_exports_the_horizon_abi():
    L = C.CDLL(ss.LIB_PATH)
    declared = ss.declared_functions()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in _capi._SIGS, name
    assert ss.lib().sunsky_abi_version() == 7
    assert hasattr(ss.SunskySequence, "irradiance_sun_columns") and callable(ss.horizon_from_elevation)
    assert "horizon_from_elevation" in ss.__all__


@pytest.mark.parametrize("variant", VARIANTS)
def test_refusals_in_the_headers_order(variant):
    """Each refusal with its message; a call that breaks several rules names the first one of the
    header's list.  The library reads no pointer before it refuses (host-only: it never does)."""
    seq = host_sequence(variant)
    L = ss.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    v3 = _capi.Vec3In(p, p, p)

    def call(nrm=v3, hz=p, sectors=4, profiles=4, hstride=4, n=4, out=p, ostride=4):
        rc = L.sunsky_sequence_irradiance_horizon(seq._h, nrm, hz, sectors, profiles, hstride, None, n, out, ostride, None)
        return rc, L.sunsky_last_error().decode()

    def refused(what, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and what in msg, (what, rc, msg)

    assert L.sunsky_sequence_irradiance_horizon(None, v3, p, 4, 4, 4, None, 4, p, 4, None) == 1
    # n == 0 succeeds before anything else is looked at
    assert call(nrm=_capi.Vec3In(None, None, None), hz=None, sectors=0, profiles=7, hstride=0, n=0, out=None)[0] == 0
    # 1-3: pointers and n, before the sequence's state (nothing is prepared yet)
    refused("null normal / output pointer", nrm=_capi.Vec3In(None, p, p), hz=None, n=1 << 32)
    refused("null normal / output pointer", out=None, hz=None)
    refused("null horizon pointer", hz=None, n=1 << 32, profiles=1 << 32, hstride=1 << 32, ostride=1 << 32)
    refused("2^32", n=1 << 32, profiles=1 << 32, hstride=1 << 32, ostride=1 << 32)
    # 4: before prepare_irradiance, whatever else is wrong
    refused("sunsky_sequence_prepare_irradiance first")
    refused("sunsky_sequence_prepare_irradiance first", sectors=0, profiles=2, hstride=0, ostride=0)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.irradiance_sun_columns()
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.irradiance(np.zeros((3, 4), np.float32), horizon=torch.zeros(4))
    seq.prepare_irradiance(8, 16, wavelengths=lam_of(variant))
    # 5: n_sectors
    for sectors in (0, -1, 3, 5, 32):
        refused("n_sectors must be >= 1 and divide", sectors=sectors, profiles=2, hstride=0, ostride=0)
    # 6: n_profiles
    for profiles in (0, 2, 3, 5):
        refused("n_profiles must be 1 or n", profiles=profiles, hstride=0, ostride=0)
    # 7: the horizon's stride, for per-receiver profiles of more than one sector
    refused("horizon_stride < n", hstride=3, ostride=0)
    refused("horizon_stride < n", hstride=0, ostride=0)
    # 8: out's stride
    refused("out_stride < n", ostride=3)
    # 9: everything in order, but host-only -- for every accepted shape
    for kw in ({}, {"sectors": 1, "hstride": 0}, {"sectors": 16}, {"profiles": 1, "hstride": 1},
               {"profiles": 1, "hstride": 0}, {"sectors": 2, "hstride": 100, "ostride": 100}, {"n": 1, "profiles": 1}):
        refused("host-only sequence", **kw)
    # the unoccluded call and the table ids are as they were
    assert L.sunsky_sequence_irradiance(seq._h, v3, None, 4, p, 4, None) == 1
    assert b"host-only sequence" in L.sunsky_last_error()
    assert L.sunsky_sequence_get_irradiance_table(seq._h, 2, None, 0, None) == 1
    assert b"unknown sequence irradiance table id" in L.sunsky_last_error()


def numpy_columns(seq, n_phi):
    """floor(phi n_phi / 2 pi) of every frame's local sun in fp64, and the distance in radians of
    phi from the nearest column boundary."""
    s = np.array([seq.frame(k)["sun_dir_local"] for k in range(len(seq))], np.float64)
    phi = np.mod(np.arctan2(s[:, 1], s[:, 0]), 2 * np.pi)
    x = phi * n_phi / (2 * np.pi)
    return np.clip(np.floor(x).astype(np.int64), 0, n_phi - 1), np.abs(x - np.round(x)) * (2 * np.pi / n_phi)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_sun_columns_against_numpy(variant, rotated):
    """j_k of the five frames (azimuths 10, 100, 200, 300 and 40 degrees; one frame of weight 0 and
    one at night, which the staged image leaves out and the getter does not) at four grids.  The
    library rounds in fp32, so a sun within 1e-4 rad of a column boundary would be excluded: the
    chosen frames have none."""
    seq = host_sequence(variant, **({"to_world": rotation()} if rotated else {}))
    for n_phi in (16, 20, 32, 256):
        seq.prepare_irradiance(3, n_phi, wavelengths=lam_of(variant))
        want, margin = numpy_columns(seq, n_phi)
        assert np.all(margin > 1e-4), margin
        got = seq.irradiance_sun_columns()
        assert got.dtype == np.int32 and got.shape == (5,)
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(want, [7, 71, 142, 213, 28])
    cnt = C.c_size_t()
    two = (C.c_int * 2)(-1, -1)
    assert ss.lib().sunsky_sequence_get_irradiance_sun_columns(seq._h, two, 2, C.byref(cnt)) == 0   # a short buffer
    assert cnt.value == 5 and list(two) == [7, 71]
    assert ss.lib().sunsky_sequence_get_irradiance_sun_columns(None, None, 0, None) == 1


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_sun_at_the_pole_has_column_0_and_update_drops_the_columns(variant):
    dirs = np.array([[0, 0, 1], [0, 1, 1], [-1, -1, 1]], np.float32)
    seq = host_sequence(variant, dirs, [2.0, 3.0, 4.0], [1.0, 1.0, 1.0])
    seq.prepare_irradiance(4, 16, wavelengths=lam_of(variant))
    assert np.all(seq.frame(0)["sun_dir_local"] == [0, 0, 1])
    np.testing.assert_array_equal(seq.irradiance_sun_columns(), [0, 4, 10])
    seq.update(sun_directions=np.array([[1, 1, 1], [0, 0, 1], [1, -1, 0.5]], np.float32))
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.irradiance_sun_columns()
    seq.prepare_irradiance(4, 8, wavelengths=lam_of(variant))
    np.testing.assert_array_equal(seq.irradiance_sun_columns(), [1, 0, 7])


def test_python_argument_checks():
    """Shapes, dtype and a sector count that does not divide n_phi are refused before any launch,
    so a host-only sequence shows them; a valid horizon reaches the host-only refusal, and
    horizon=None is the call it always was."""
    seq = host_sequence("rgb")
    seq.prepare_irradiance(8, 16)
    nrm = np.zeros((3, 4), np.float32)
    for bad in (np.zeros(4, np.float32), [0.0] * 4, torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="horizon must be a float32 tensor"):
            seq.irradiance(nrm, horizon=bad)
    for shape in ((), (0,), (4, 2), (4, 3), (4, 5), (4, 4, 1), (0, 4)):
        with pytest.raises(ValueError, match="horizon must have shape"):
            seq.irradiance(nrm, horizon=torch.zeros(shape))
    for sectors in (3, 5, 32):
        with pytest.raises(ValueError, match=f"{sectors} sectors do not divide the irradiance tables' n_phi = 16"):
            seq.irradiance(nrm, horizon=torch.zeros(sectors))
        with pytest.raises(ValueError, match="do not divide"):
            seq.irradiance(nrm, horizon=torch.zeros(sectors, 4))
    for good in (torch.zeros(4), torch.zeros(16, 1), torch.zeros(2, 4), torch.zeros(1), None):
        with pytest.raises(ValueError, match="host-only"):
            seq.irradiance(nrm, horizon=good)


def test_horizon_from_elevation():
    deg = [0.0, 10.0, 30.0, 90.0, -5.0]
    want = np.sin(np.deg2rad(np.asarray(deg, np.float64))).astype(np.float32)
    h = ss.horizon_from_elevation(deg)
    assert isinstance(h, np.ndarray) and h.dtype == np.float32
    np.testing.assert_array_equal(h, want)
    assert h[0] == 0 and h[2] == np.float32(0.5) and h[3] == 1 and h[4] < 0
    t = ss.horizon_from_elevation(torch.tensor([deg, deg], dtype=torch.float32))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == (2, 5)
    np.testing.assert_array_equal(t.numpy(), np.stack([want, want]))
    assert ss.horizon_from_elevation(30.0).shape == () and ss.horizon_from_elevation(30.0) == np.float32(0.5)
