"""Frame sequences (sunsky_sequence_*, sunsky_amd.SunskySequence) without a GPU: the ABI
additions, sunsky_sun_coordinates, host-only sequences against single host emitters, and the
validation messages."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import sunsky_amd as ss
from sunsky_amd import _capi
from helpers import hour_dict
from sequence_cases import ELEVATIONS, TURBIDITY, WEIGHTS, base_dict, frame_dict, frame_dirs, rotation

NEW_SYMBOLS = ["sunsky_sun_coordinates", "sunsky_sequence_create", "sunsky_sequence_destroy", "sunsky_sequence_info",
               "sunsky_sequence_set_precision", "sunsky_sequence_get_frame", "sunsky_sequence_eval",
               "sunsky_sequence_bake_latlong"]


def test_library_exports_the_sequence_abi():
    L = C.CDLL(ss.LIB_PATH)
    declared = ss.declared_functions()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in _capi._SIGS, name
    assert ss.lib().sunsky_abi_version() == 7
    for name in ("SunskySequence", "sun_coordinates"):
        assert name in ss.__all__ and hasattr(ss, name)


@pytest.mark.parametrize("hd", [hour_dict(3, 11.7753, 0.1, 1.0, 1.0), hour_dict(5.2, 9.5, 0.2, 1.0, 1.0),
                                hour_dict(3, 12.0, 0.2, 1.0, 1.0)])
def test_sun_coordinates_match_oracle_and_the_time_location_emitter(hd):
    s = ss.sun_coordinates(2010, 7, 10, hd["hour"])
    np.testing.assert_allclose(s, O.sun_coordinates(hour=hd["hour"]), rtol=0, atol=2e-7)
    em = ss.SunskyEmitter(hd, device="host")
    np.testing.assert_array_equal(s, em.info()["sun_dir_world"].astype(np.float32))


def test_sun_coordinates_other_date_and_place():
    s = ss.sun_coordinates(2024, 12, 21, 9.0, 30.0, 15.0, latitude=48.85, longitude=2.35, timezone=1.0)
    ref = O.sun_coordinates(year=2024, month=12, day=21, hour=9.0, minute=30.0, second=15.0, latitude=48.85,
                            longitude=2.35, timezone=1.0)
    np.testing.assert_allclose(s, ref, rtol=0, atol=2e-7)


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
@pytest.mark.parametrize("rotated", [False, True])
def test_host_sequence_frames_equal_single_host_emitters(variant, rotated):
    base = base_dict(**({"to_world": rotation()} if rotated else {}))
    parent = ss.SunskyEmitter(base, variant=variant, device="host")
    dirs = frame_dirs(rotation() if rotated else None)
    seq = ss.SunskySequence(parent, dirs, TURBIDITY, WEIGHTS)
    nch = 11 if variant == "spectral" else 3
    assert seq.info() == {"count": 5, "variant": 1 if variant == "spectral" else 0, "nb_channels": nch,
                          "precision": "fast", "device": -1}
    assert len(seq) == 5
    for k in range(5):
        single = ss.SunskyEmitter(frame_dict(base, dirs[k], TURBIDITY[k]), variant=variant, device="host")
        f = seq.frame(k)
        np.testing.assert_array_equal(f["sky_params"].reshape(-1), single.table("sky_params"))
        np.testing.assert_array_equal(f["sky_radiance"], single.table("sky_radiance"))
        np.testing.assert_array_equal(f["sun_dir_local"], single.info()["sun_dir_local"].astype(np.float32))
        assert f["weight"] == np.float32(WEIGHTS[k]) and f["turbidity"] == np.float32(TURBIDITY[k])
        assert np.any(f["sky_params"] != 0) == (ELEVATIONS[k] >= 0)   # a sun below the horizon stages zeros
    # the snapshot: the parent's later updates do not reach the sequence
    before = seq.frame(1)
    p = parent.traverse()
    p["albedo"] = 0.9
    p.update()
    np.testing.assert_array_equal(seq.frame(1)["sky_params"], before["sky_params"])
    del parent
    np.testing.assert_array_equal(seq.frame(1)["sky_params"], before["sky_params"])


def test_defaults_scalar_turbidity_and_precision():
    parent = ss.SunskyEmitter(base_dict(), device="host")
    seq = ss.SunskySequence(parent, frame_dirs()[:2])
    assert [seq.frame(k)["turbidity"] for k in range(2)] == [4.0, 4.0]
    assert [seq.frame(k)["weight"] for k in range(2)] == [1.0, 1.0]
    seq = ss.SunskySequence(parent, frame_dirs()[:2], turbidity=2.0)
    assert seq.frame(1)["turbidity"] == 2.0
    seq.set_precision("reference")
    assert seq.info()["precision"] == "reference"
    with pytest.raises(KeyError):
        seq.set_precision("half")
    with pytest.raises(ValueError, match="frame index"):
        seq.frame(2)


def test_from_times_uses_sun_coordinates():
    parent = ss.SunskyEmitter(base_dict(to_world=rotation()), device="host")
    times = [(2010, 7, 10, h) for h in range(24)]
    seq = ss.SunskySequence.from_times(parent, times, latitude=35.6894, longitude=139.6917, timezone=9.0,
                                       weights=np.arange(24) / 10.0)
    assert len(seq) == 24
    below = 0
    for h in (0, 6, 12, 15, 23):
        s = ss.sun_coordinates(2010, 7, 10, float(h))
        # local = to_local (to_world s): the rotation round trip, a few ulps
        np.testing.assert_allclose(seq.frame(h)["sun_dir_local"], s, rtol=0, atol=5e-7)
        below += s[2] < 0
    assert below >= 2   # the day includes night hours


def test_validation_messages():
    parent = ss.SunskyEmitter(base_dict(), device="host")
    d = frame_dirs()[:1]
    with pytest.raises(ValueError, match="at least one frame"):
        ss.SunskySequence(parent, np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match=r"Turbidity value 12\.000000 is out of range \[1, 10\]"):
        ss.SunskySequence(parent, d, turbidity=[12.0])
    with pytest.raises(ValueError, match="Turbidity value"):
        ss.SunskySequence(parent, d, turbidity=[float("nan")])
    with pytest.raises(ValueError, match="sun direction must be finite and non-zero"):
        ss.SunskySequence(parent, np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError, match="sun direction must be finite and non-zero"):
        ss.SunskySequence(parent, np.array([[0.0, np.inf, 1.0]], np.float32))
    with pytest.raises(ValueError, match="weight must be finite and >= 0"):
        ss.SunskySequence(parent, d, weights=[float("nan")])
    with pytest.raises(ValueError, match="weight must be finite and >= 0"):
        ss.SunskySequence(parent, d, weights=[-0.5])
    # the C ABI's own status for each
    L, h = ss.lib(), C.c_void_p()
    one = (C.c_float * 3)(0.0, 0.0, 1.0)
    for args in [(0, one, None, None), (1, one, (C.c_float * 1)(12.0), None), (1, (C.c_float * 3)(), None, None),
                 (1, one, None, (C.c_float * 1)(float("nan"))), (1, one, None, (C.c_float * 1)(-1.0))]:
        assert L.sunsky_sequence_create(parent._h, *args, C.byref(h)) == 1   # SUNSKY_ERROR_INVALID_VALUE
        assert not h.value


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_batch_calls_on_a_host_only_sequence_fail_cleanly(variant):
    parent = ss.SunskyEmitter(base_dict(), variant=variant, device="host")
    seq = ss.SunskySequence(parent, frame_dirs())
    with pytest.raises(ValueError, match="host-only"):
        seq.eval(np.zeros((3, 4), np.float32), wavelengths=[550.0] if variant == "spectral" else None)
    with pytest.raises(ValueError, match="host-only"):
        seq.bake_latlong(8, 4, wavelengths=[550.0] if variant == "spectral" else None)
    # and through the C ABI (the pointers are never read: the call is refused first)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    lam = (C.c_float * 1)(550.0) if variant == "spectral" else None
    m = 1 if variant == "spectral" else 0
    rc = ss.lib().sunsky_sequence_eval(seq._h, _capi.Vec3In(p, p, p), lam, m, None, 4, p, 4, None)
    assert rc == 1 and b"host-only sequence" in ss.lib().sunsky_last_error()
    rc = ss.lib().sunsky_sequence_bake_latlong(seq._h, 2, 2, 0.0, 1.0, 0.0, 1.0, lam, m, p, 4, None)
    assert rc == 1 and b"host-only sequence" in ss.lib().sunsky_last_error()
