"""The per-frame irradiance series without a GPU (host-only sequences): the ABI additions, a
frame's own sky table bit for bit against one-frame sequences and against the weighted table,
every refusal of sunsky_sequence_irradiance_series in the header's order, the life cycle of the
preparation (sticky across prepare_irradiance, dropped by update), the cap, and the Python
argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import sunsky_amd as ss
from sunsky_amd import _capi
from sequence_cases import LAMBDAS, TURBIDITY, WEIGHTS, base_dict, frame_dirs, rotation

NEW_SYMBOLS = ["sunsky_sequence_prepare_irradiance_series", "sunsky_sequence_get_irradiance_frame_table",
               "sunsky_sequence_irradiance_series"]
VARIANTS = ["rgb", "spectral"]
NOT_PREPARED = "sunsky_sequence_prepare_irradiance_series first"


def lam_of(variant):
    return LAMBDAS if variant == "spectral" else None


def host_parent(variant, **kw):
    return ss.SunskyEmitter(base_dict(**kw), variant=variant, device="host")


def host_sequence(variant, dirs=None, turb=TURBIDITY, wts=WEIGHTS, **kw):
    return ss.SunskySequence(host_parent(variant, **kw), frame_dirs(kw.get("to_world")) if dirs is None else dirs, turb, wts)


def fma32(w, t, acc):
    """fma(w, t, acc) in fp32, exactly: the fp64 product of two fp32 values is exact; its fp64 sum
    with acc is rounded to odd (TwoSum gives the sum's exact error), after which the rounding to
    fp32 is that of the exact value."""
    p = np.float64(w) * t.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    b = s - p
    err = (p - (s - b)) + (a - b)
    even = (s.view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, odd, s).astype(np.float32)


def test_library_exports_the_series_abi():
    L = C.CDLL(ss.LIB_PATH)
    declared = ss.declared_functions()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in _capi._SIGS, name
    assert ss.lib().sunsky_abi_version() == 7
    for method in ("prepare_irradiance_series", "irradiance_frame_table", "irradiance_series"):
        assert callable(getattr(ss.SunskySequence, method))
    # G is a function of the plane count alone: 8 frames for RGB, one for the widest list
    assert [_capi.seq_irr_series_group(p) for p in (1, 2, 3, 4, 5, 8, 12, 13, 24, 25, 32)] == [8, 8, 8, 6, 4, 3, 2, 1, 1, 1, 1]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("rotated", [False, True])
def test_frame_tables_are_the_one_frame_sequences_tables(variant, rotated):
    """irradiance_frame_table(k) of all five frames bit for bit the "sky" table of the one-frame,
    weight-1 sequence; the weighted sequence's table bit for bit the frame-order accumulation
    fma(w_k, frame_table_k, acc) (fp32, the fma exact through fp64); the night frame's table and
    the 300 nm plane exactly 0."""
    kw = {"to_world": rotation()} if rotated else {}
    seq = host_sequence(variant, **kw)
    dirs = frame_dirs(kw.get("to_world"))
    for size in ((3, 20), (8, 16)):
        seq.prepare_irradiance(*size, wavelengths=lam_of(variant))
        planes = seq.irradiance_info()["n_planes"]
        acc = np.zeros((planes,) + size, np.float32)
        for k in range(5):
            t = seq.irradiance_frame_table(k)
            assert t.dtype == np.float32 and t.shape == (planes,) + size
            one = ss.SunskySequence(host_parent(variant, **kw), dirs[k:k + 1], TURBIDITY[k:k + 1], [1.0])
            one.prepare_irradiance(*size, wavelengths=lam_of(variant))
            want = one.irradiance_table("sky")
            assert t.tobytes() == want.tobytes(), (variant, rotated, size, k)
            acc = fma32(np.float32(WEIGHTS[k]), t, acc)
            if k == 4:
                assert np.all(t == 0)
            else:
                assert np.all(t >= 0) and np.all(t[:3].max((1, 2)) > 0)
            if variant == "spectral":
                assert np.all(t[4] == 0)
        assert acc.tobytes() == seq.irradiance_table("sky").tobytes(), (variant, rotated, size)


@pytest.mark.parametrize("variant", VARIANTS)
def test_frame_table_getter_conventions(variant):
    seq = host_sequence(variant)
    L = ss.lib()
    cnt = C.c_size_t()
    assert L.sunsky_sequence_get_irradiance_frame_table(None, 0, None, 0, None) == 1
    assert L.sunsky_sequence_get_irradiance_frame_table(seq._h, 0, None, 0, C.byref(cnt)) == 1
    assert b"sunsky_sequence_prepare_irradiance first" in L.sunsky_last_error()
    seq.prepare_irradiance(3, 20, wavelengths=lam_of(variant))
    planes = seq.irradiance_info()["n_planes"]
    for k in (-1, 5):
        assert L.sunsky_sequence_get_irradiance_frame_table(seq._h, k, None, 0, C.byref(cnt)) == 1
        assert b"frame index out of range" in L.sunsky_last_error()
    assert L.sunsky_sequence_get_irradiance_frame_table(seq._h, 1, None, 0, C.byref(cnt)) == 0 and cnt.value == planes * 60
    two = (C.c_float * 3)(-1.0, -1.0, -1.0)   # a short buffer is filled up to its capacity
    assert L.sunsky_sequence_get_irradiance_frame_table(seq._h, 1, two, 2, C.byref(cnt)) == 0 and cnt.value == planes * 60
    full = seq.irradiance_frame_table(1).reshape(-1)
    assert list(two) == [full[0], full[1], -1.0]
    # the weighted tables' ids are as they were
    assert L.sunsky_sequence_get_irradiance_table(seq._h, 2, None, 0, None) == 1
    assert b"unknown sequence irradiance table id" in L.sunsky_last_error()
    # works without prepare_irradiance_series, and update drops it with the tables
    seq.update(weights=[1.0] * 5)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.irradiance_frame_table(0)


@pytest.mark.parametrize("variant", VARIANTS)
def test_refusals_in_the_headers_order(variant):
    """Each refusal with its message; a call that breaks several rules names the first one of the
    header's list.  The library reads no pointer before it refuses (host-only: it never does)."""
    seq = host_sequence(variant)
    L = ss.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    v3 = _capi.Vec3In(p, p, p)

    def call(nrm=v3, hz=None, sectors=4, profiles=4, hstride=4, n=4, first=0, frames=5, out=p, ostride=4):
        rc = L.sunsky_sequence_irradiance_series(seq._h, nrm, hz, sectors, profiles, hstride, None, n, first, frames, out,
                                                 ostride, None)
        return rc, L.sunsky_last_error().decode()

    def refused(what, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and what in msg, (what, rc, msg)

    assert L.sunsky_sequence_irradiance_series(None, v3, None, 0, 0, 0, None, 4, 0, 5, p, 4, None) == 1
    assert L.sunsky_sequence_prepare_irradiance_series(None) == 1
    # n == 0 or n_frames == 0 succeeds before anything else is looked at
    nothing = dict(nrm=_capi.Vec3In(None, None, None), hz=p, sectors=0, profiles=7, hstride=0, out=None, ostride=0)
    assert call(n=0, first=-3, frames=99, **nothing)[0] == 0
    assert call(n=1 << 33, first=-3, frames=0, **nothing)[0] == 0
    # 1-2: pointers and n, before the sequence's state (nothing is prepared yet)
    refused("null normal / output pointer", nrm=_capi.Vec3In(p, None, p), n=1 << 32, first=-1)
    refused("null normal / output pointer", out=None, n=1 << 32)
    refused("2^32", n=1 << 32, first=-1, ostride=0)
    # 3: before prepare_irradiance_series, whatever else is wrong -- also with the tables prepared
    refused(NOT_PREPARED)
    refused(NOT_PREPARED, first=-1, frames=99, hz=p, sectors=0, ostride=0)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.prepare_irradiance_series()
    seq.prepare_irradiance(8, 16, wavelengths=lam_of(variant))
    refused(NOT_PREPARED, first=-1, frames=99, hz=p, sectors=0, ostride=0)
    with pytest.raises(ValueError, match=NOT_PREPARED):
        seq.irradiance_series(np.zeros((3, 4), np.float32))
    seq.prepare_irradiance_series()
    # 4: the frame range
    for first, frames in ((-1, 1), (0, -1), (0, 6), (5, 1), (3, 3), (2 ** 31 - 1, 2 ** 31 - 1)):
        refused("frame range out of range", first=first, frames=frames, hz=p, sectors=0, ostride=0)
    # 5: with a horizon, irradiance_horizon's three refusals in its wording
    for sectors in (0, -1, 3, 5, 32):
        refused("n_sectors must be >= 1 and divide", hz=p, sectors=sectors, profiles=2, hstride=0, ostride=0)
    for profiles in (0, 2, 3, 5):
        refused("n_profiles must be 1 or n", hz=p, profiles=profiles, hstride=0, ostride=0)
    refused("horizon_stride < n", hz=p, hstride=3, ostride=0)
    refused("horizon_stride < n", hz=p, hstride=0, ostride=0)
    # ... which a NULL horizon ignores
    refused("out_stride < n", sectors=0, profiles=7, hstride=0, ostride=3)
    # 6: out's stride, with more than one output plane
    refused("out_stride < n", ostride=3)
    refused("out_stride < n", hz=p, ostride=0)
    refused("out_stride < n", first=4, frames=1, ostride=3)
    # 7: everything in order, but host-only -- for every accepted shape
    for kw in ({}, {"first": 4, "frames": 1}, {"first": 2, "frames": 3}, {"hz": p}, {"hz": p, "sectors": 1, "hstride": 0},
               {"hz": p, "profiles": 1, "hstride": 0}, {"hz": p, "sectors": 2, "hstride": 100, "ostride": 100},
               {"n": 1, "hz": p, "profiles": 1}, {"sectors": -5, "profiles": 0, "hstride": 0}):
        refused("host-only sequence", **kw)
    # the calls next to it are as they were
    assert L.sunsky_sequence_irradiance(seq._h, v3, None, 4, p, 4, None) == 1
    assert b"host-only sequence" in L.sunsky_last_error()


def test_a_single_output_plane_needs_no_stride():
    """One wavelength and one frame: one output plane, so out_stride is not looked at."""
    seq = host_sequence("spectral")
    seq.prepare_irradiance(3, 20, wavelengths=[550.0])
    seq.prepare_irradiance_series()
    L = ss.lib()
    p = C.cast((C.c_float * 16)(), C.c_void_p)
    v3 = _capi.Vec3In(p, p, p)
    assert L.sunsky_sequence_irradiance_series(seq._h, v3, None, 0, 0, 0, None, 4, 2, 1, p, 0, None) == 1
    assert b"host-only sequence" in L.sunsky_last_error()
    assert L.sunsky_sequence_irradiance_series(seq._h, v3, None, 0, 0, 0, None, 4, 2, 2, p, 0, None) == 1
    assert b"out_stride < n" in L.sunsky_last_error()


@pytest.mark.parametrize("variant", VARIANTS)
def test_preparation_is_sticky_and_update_drops_it(variant):
    seq = host_sequence(variant)
    L = ss.lib()
    p = C.cast((C.c_float * 64)(), C.c_void_p)
    v3 = _capi.Vec3In(p, p, p)

    def series():
        rc = L.sunsky_sequence_irradiance_series(seq._h, v3, None, 0, 0, 0, None, 4, 0, 5, p, 4, None)
        return rc, L.sunsky_last_error().decode()

    lam = lam_of(variant)
    seq.prepare_irradiance(8, 16, wavelengths=lam)
    seq.prepare_irradiance_series()
    assert "host-only sequence" in series()[1]
    # sticky: new tables restage it
    seq.prepare_irradiance(16, 32, wavelengths=lam)
    assert "host-only sequence" in series()[1]
    # update drops it together with the tables; prepare_irradiance alone brings both back
    seq.update(weights=[1.0, 1.0, 0.0, 1.0, 1.0])
    rc, msg = series()
    assert rc == 1 and NOT_PREPARED in msg
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_irradiance first"):
        seq.prepare_irradiance_series()
    seq.prepare_irradiance(3, 20, wavelengths=lam)
    assert "host-only sequence" in series()[1]
    # independent of the gradients' preparation
    other = host_sequence(variant)
    other.prepare_irradiance(3, 20, wavelengths=lam)
    other.prepare_irradiance_grad()
    with pytest.raises(ValueError, match=NOT_PREPARED):
        other.irradiance_series(np.zeros((3, 4), np.float32))
    other.prepare_irradiance_series()
    with pytest.raises(ValueError, match="host-only"):
        other.irradiance_series(np.zeros((3, 4), np.float32))


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_lowered_cap_refuses(variant, monkeypatch):
    """K P Q floats against the cap as the environment lowers it, read at every prepare: one
    below refuses with a message, exactly at the cap passes.  A restaging above the cap leaves the
    series unprepared."""
    seq = host_sequence(variant)
    seq.prepare_irradiance(3, 20, wavelengths=lam_of(variant))
    need = 5 * seq.irradiance_info()["n_planes"] * 60
    assert _capi.SEQ_IRR_SERIES_MAX_ENV == "SUNSKY_AMD_IRRADIANCE_SERIES_MAX_FLOATS" and _capi.SEQ_IRR_SERIES_MAX_FLOATS == 1 << 26
    monkeypatch.setenv(_capi.SEQ_IRR_SERIES_MAX_ENV, str(need - 1))
    with pytest.raises(ValueError, match=f"exceeds the cap of {need - 1} floats"):
        seq.prepare_irradiance_series()
    with pytest.raises(ValueError, match=NOT_PREPARED):
        seq.irradiance_series(np.zeros((3, 4), np.float32))
    monkeypatch.setenv(_capi.SEQ_IRR_SERIES_MAX_ENV, str(need))
    seq.prepare_irradiance_series()
    with pytest.raises(ValueError, match="host-only"):
        seq.irradiance_series(np.zeros((3, 4), np.float32))
    seq.prepare_irradiance(8, 16, wavelengths=lam_of(variant))   # larger tables: the restaging does not fit
    with pytest.raises(ValueError, match=NOT_PREPARED):
        seq.irradiance_series(np.zeros((3, 4), np.float32))
    monkeypatch.setenv(_capi.SEQ_IRR_SERIES_MAX_ENV, str(1 << 40))   # the variable only lowers the cap
    seq.prepare_irradiance_series()
    monkeypatch.delenv(_capi.SEQ_IRR_SERIES_MAX_ENV)
    seq.prepare_irradiance_series()


def test_python_argument_checks():
    """frames= is checked before any launch, so a host-only sequence shows it; valid arguments
    reach the host-only refusal."""
    seq = host_sequence("rgb")
    seq.prepare_irradiance(8, 16)
    seq.prepare_irradiance_series()
    nrm = np.zeros((3, 4), np.float32)
    for bad in (3, "ab", (1,), (1, 2, 3), (0.0, 2), (0, 2.5), [True, 1], range(0, 4, 2), range(4, 0, -1), {"first": 0}):
        with pytest.raises(ValueError, match="frames must be None, a \\(first, count\\) pair or a range with step 1"):
            seq.irradiance_series(nrm, frames=bad)
    for bad in ((-1, 2), (0, 6), (5, 1), (3, -1), range(3, 7), range(-1, 2)):
        with pytest.raises(ValueError, match="are not within the sequence's 5 frames"):
            seq.irradiance_series(nrm, frames=bad)
    for good in (None, (0, 5), (4, 1), [2, 3], (5, 0), range(5), range(2, 4), range(3, 3), (np.int64(1), np.int32(2))):
        with pytest.raises(ValueError, match="host-only"):
            seq.irradiance_series(nrm, frames=good)
    assert seq._frames(range(2, 4)) == (2, 2) and seq._frames(None) == (0, 5) and seq._frames(range(3, 3)) == (0, 0)
    with pytest.raises(ValueError, match="host-only"):
        seq.irradiance_series(nrm, horizon=torch.zeros(4))
