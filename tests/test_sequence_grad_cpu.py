"""Per-frame gradients and the in-place update of a frame sequence without a GPU: the ABI
additions, update against a freshly created host-only sequence, the gradient records against
single host emitters' tangent tables, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import sunsky_amd as ss
from sunsky_amd import _capi
from sequence_cases import ELEVATIONS, TURBIDITY, WEIGHTS, base_dict, frame_dict, frame_dirs, rotation

NEW_SYMBOLS = ["sunsky_sequence_update", "sunsky_sequence_prepare_grad", "sunsky_sequence_get_frame_tangent",
               "sunsky_sequence_eval_vjp"]
OTHER_T, OTHER_W = [2.0, 3.5, 4.0, 9.0, 1.5], [1.0, 0.0, 0.25, 4.0, 2.0]


def test_library_exports_the_sequence_gradient_abi():
    L = C.CDLL(ss.LIB_PATH)
    declared = ss.declared_functions()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in _capi._SIGS, name
    assert ss.lib().sunsky_abi_version() == 7
    assert "sequence_eval" in ss.__all__ and callable(ss.sequence_eval)
    for name in ("update", "prepare_grad", "frame_tangent", "eval_vjp"):
        assert callable(getattr(ss.SunskySequence, name))


def same_frames(a, b):
    assert len(a) == len(b)
    for k in range(len(a)):
        fa, fb = a.frame(k), b.frame(k)
        for key in ("sun_dir_local", "sky_params", "sky_radiance"):
            np.testing.assert_array_equal(fa[key], fb[key])
        assert fa["weight"] == fb["weight"] and fa["turbidity"] == fb["turbidity"]


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
@pytest.mark.parametrize("rotated", [False, True])
def test_update_equals_a_freshly_created_sequence(variant, rotated):
    tw = rotation() if rotated else None
    parent = ss.SunskyEmitter(base_dict(**({"to_world": tw} if rotated else {})), variant=variant, device="host")
    dirs = frame_dirs(tw)
    seq = ss.SunskySequence(parent, dirs[::-1].copy())   # other suns, the parent's turbidity, weight 1
    seq.update(dirs, TURBIDITY, WEIGHTS)
    same_frames(seq, ss.SunskySequence(parent, dirs, TURBIDITY, WEIGHTS))
    seq.update(turbidity=OTHER_T)                         # None keeps the current values
    same_frames(seq, ss.SunskySequence(parent, dirs, OTHER_T, WEIGHTS))
    seq.update(weights=OTHER_W)
    same_frames(seq, ss.SunskySequence(parent, dirs, OTHER_T, OTHER_W))
    seq.update(sun_directions=2.5 * dirs[::-1])
    same_frames(seq, ss.SunskySequence(parent, 2.5 * dirs[::-1], OTHER_T, OTHER_W))
    del parent                                            # the sequence restages from its own copies
    seq.update(dirs, 3.0, WEIGHTS)
    assert [seq.frame(k)["turbidity"] for k in range(5)] == [3.0] * 5


def test_update_validation_and_a_refused_update():
    parent = ss.SunskyEmitter(base_dict(), device="host")
    dirs = frame_dirs()
    seq = ss.SunskySequence(parent, dirs, TURBIDITY, WEIGHTS)
    fresh = ss.SunskySequence(parent, dirs, TURBIDITY, WEIGHTS)
    bad_dir, inf_dir = dirs.copy(), dirs.copy()
    bad_dir[3] = 0.0
    inf_dir[2, 1] = np.inf
    refusals = [
        (dict(turbidity=[1.0, 2.0, 12.0, 3.0, 4.0]), r"Turbidity value 12\.000000 is out of range \[1, 10\] \(frame 2\)"),
        (dict(turbidity=[float("nan")] * 5), "Turbidity value"),
        (dict(sun_directions=bad_dir), "frame 3: the sun direction must be finite and non-zero"),
        (dict(sun_directions=inf_dir), "frame 2: the sun direction must be finite and non-zero"),
        (dict(weights=[1.0, float("nan"), 1.0, 1.0, 1.0]), "frame 1: the weight must be finite and >= 0"),
        (dict(weights=[1.0, 1.0, 1.0, 1.0, -0.5]), "frame 4: the weight must be finite and >= 0"),
        # valid arrays beside the refused one are not taken either
        (dict(sun_directions=dirs[::-1].copy(), turbidity=OTHER_T, weights=[-1.0] * 5), "weight must be finite"),
    ]
    for kw, message in refusals:
        with pytest.raises(ValueError, match=message):
            seq.update(**kw)
        same_frames(seq, fresh)
    with pytest.raises(ValueError, match="keeps the frame count"):
        seq.update(sun_directions=dirs[:4])
    with pytest.raises(ValueError, match="must have 5 values"):
        seq.update(turbidity=[1.0, 2.0])
    same_frames(seq, fresh)
    # the C ABI's own status
    assert ss.lib().sunsky_sequence_update(None, None, None, None) == 1
    assert ss.lib().sunsky_sequence_update(seq._h, None, (C.c_float * 5)(1, 2, 3, 4, 11), None) == 1
    assert b"(frame 4)" in ss.lib().sunsky_last_error()
    assert ss.lib().sunsky_sequence_update(seq._h, None, None, None) == 0   # nothing given: the same frames again
    same_frames(seq, fresh)


def test_update_drops_the_sampling_distribution():
    parent = ss.SunskyEmitter(base_dict(), device="host")
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    seq.prepare_sampling(8, 16)
    assert seq.sampling_info()["n_z"] == 8
    seq.update(weights=OTHER_W)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_sampling first"):
        seq.sampling_info()
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_sampling first"):
        seq.sampling_table("q")
    seq.prepare_sampling(8, 16)
    fresh = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, OTHER_W)
    fresh.prepare_sampling(8, 16)
    for name in ("sky", "q", "B", "frame_cdf"):
        np.testing.assert_array_equal(seq.sampling_table(name), fresh.sampling_table(name))


def axis_tangent(s, a):
    """(I - s^ s^T) e_a / |s| in fp32: the world tangent of the normalised direction along axis a."""
    s = np.asarray(s, np.float64)
    length = np.linalg.norm(s)
    u = s / length
    return ((np.eye(3)[a] - u * u[a]) / length).astype(np.float32)


def close(a, b, what):
    """1e-6 of the block's largest magnitude: two fp32 roundings."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), np.abs(a).max())
    assert np.abs(a - b).max() <= 1e-6 * scale, (what, np.abs(a - b).max(), scale)


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("length", [1.0, 2.5])
def test_frame_tangents_against_single_host_emitters(variant, rotated, length):
    """dsky_turbidity bit for bit the single emitter's turbidity tangent table; deta[a] x
    dsky_elevation and dsun_local[a] its sun_direction tables along (I - s^ s^T) e_a / |s|.
    Directions of length 2.5: the single emitter takes the normalised direction, the records
    scale by 1 / 2.5 and have no component along s."""
    tw = rotation() if rotated else None
    base = base_dict(**({"to_world": tw} if rotated else {}))
    parent = ss.SunskyEmitter(base, variant=variant, device="host")
    unit = frame_dirs(tw)
    dirs = (length * unit).astype(np.float32)
    seq = ss.SunskySequence(parent, dirs, TURBIDITY, WEIGHTS)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_grad first"):
        seq.frame_tangent(0)
    seq.prepare_grad()
    with pytest.raises(ValueError, match="frame index"):
        seq.frame_tangent(5)
    unit_seq = ss.SunskySequence(parent, unit, TURBIDITY, WEIGHTS)
    unit_seq.prepare_grad()
    for k in range(5):
        t = seq.frame_tangent(k)
        # the emitter whose local sun has the frame's bits: the direction as the sequence normalises it
        single = ss.SunskyEmitter(frame_dict(base, dirs[k], TURBIDITY[k]), variant=variant, device="host")
        np.testing.assert_array_equal(single.info()["sun_dir_local"].astype(np.float32), seq.frame(k)["sun_dir_local"])
        ref_t = single.tangent_tables("turbidity", [1.0], on_device=False)
        np.testing.assert_array_equal(t["dsky_turbidity"], ref_t["dsky"])
        for a in range(3):
            ref_s = single.tangent_tables("sun_direction", axis_tangent(dirs[k], a), on_device=False)
            close(t["deta"][a] * t["dsky_elevation"].astype(np.float64), ref_s["dsky"], (k, a, "dsky"))
            close(t["dsun_local"][a], ref_s["dsun_local"], (k, a, "dsun_local"))
        below = ELEVATIONS[k] < 0
        assert np.all(t["dsky_turbidity"] == 0) == below and np.all(t["dsky_elevation"] == 0) == below
        # no radial component, and 1 / |s| against the unit-length sequence
        s_hat = dirs[k].astype(np.float64) / np.linalg.norm(dirs[k].astype(np.float64))
        assert np.abs(s_hat @ t["dsun_local"].astype(np.float64)).max() <= 1e-6 / length
        assert abs(s_hat @ t["deta"].astype(np.float64)) <= 1e-6 / length
        u = unit_seq.frame_tangent(k)
        close(length * t["dsun_local"].astype(np.float64), u["dsun_local"], (k, "1/|s| dsun_local"))
        # (deta is held to the single emitter above: near the zenith it is too sensitive to the
        # last bit of the local sun for a comparison between two differently normalised suns)


def test_update_restages_the_gradient_records():
    parent = ss.SunskyEmitter(base_dict(), device="host")
    dirs = frame_dirs()
    seq = ss.SunskySequence(parent, dirs[::-1].copy())
    seq.prepare_grad()
    seq.update(dirs, TURBIDITY, WEIGHTS)
    fresh = ss.SunskySequence(parent, dirs, TURBIDITY, WEIGHTS)
    fresh.prepare_grad()
    for k in range(5):
        a, b = seq.frame_tangent(k), fresh.frame_tangent(k)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key])


@pytest.mark.parametrize("variant", ["rgb", "spectral"])
def test_eval_vjp_refusals(variant):
    """Before prepare_grad, on a host-only sequence, and with a NULL d_out."""
    parent = ss.SunskyEmitter(base_dict(), variant=variant, device="host")
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    lam_py = [550.0] if variant == "spectral" else None
    wi, d = np.zeros((3, 4), np.float32), np.zeros((1 if variant == "spectral" else 3, 4), np.float32)
    with pytest.raises(ValueError, match="sunsky_sequence_prepare_grad first"):
        seq.eval_vjp(wi, d, lam_py)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    v = _capi.Vec3In(p, p, p)
    lam = (C.c_float * 1)(550.0) if variant == "spectral" else None
    m = 1 if variant == "spectral" else 0
    L = ss.lib()
    assert L.sunsky_sequence_eval_vjp(seq._h, v, lam, m, None, 4, p, 4, p, p, p, None) == 1
    assert b"sunsky_sequence_prepare_grad first" in L.sunsky_last_error()
    seq.prepare_grad()
    with pytest.raises(ValueError, match="host-only"):
        seq.eval_vjp(wi, d, lam_py)
    assert L.sunsky_sequence_eval_vjp(seq._h, v, lam, m, None, 4, p, 4, p, p, p, None) == 1
    assert b"host-only sequence" in L.sunsky_last_error()
    assert L.sunsky_sequence_eval_vjp(seq._h, v, lam, m, None, 4, None, 4, p, p, p, None) == 1
    assert b"null cotangent" in L.sunsky_last_error()
    assert L.sunsky_sequence_eval_vjp(seq._h, v, lam, m, None, 4, p, 3, p, p, p, None) == 1
    assert L.sunsky_sequence_eval_vjp(seq._h, v, lam, m, None, 0, None, 0, p, p, p, None) == 0   # n == 0 writes nothing
    assert L.sunsky_sequence_eval_vjp(None, v, lam, m, None, 4, p, 4, p, p, p, None) == 1
    bad = (None, 0) if variant == "spectral" else ((C.c_float * 1)(550.0), 1)
    assert L.sunsky_sequence_eval_vjp(seq._h, v, bad[0], bad[1], None, 4, p, 4, p, p, p, None) == 1
