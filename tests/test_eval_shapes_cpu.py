"""CPU side of tests/test_gpu_eval_shapes.py: self-checks of the bake reference and of the input
generators (eval_shapes_reference.py), the fp32 oracle alone on the bound and the loose caps the
GPU tests hold the bake to, a bake that is wrong by one column against the same bound, and every
refusal of the eval and bake entry points that needs no device (a host-only emitter: the
arguments are checked before any device work)."""
import ctypes
import math

import numpy as np
import pytest

import eval_shapes_reference as R
import sunsky_amd as ss

VF = pytest.mark.parametrize("variant,frame", [(v, f) for v in ("rgb", "spectral") for f in R.FRAMES],
                             ids=[f"{v}-{f}" for v in ("rgb", "spectral") for f in R.FRAMES])


def _ulp_distance(a, b):
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


# ---------------------------------------------------------------- the reference's self-checks
def test_fma_rounds_once():
    """fma_f32 against cases where an fp64 sum rounded to fp32 rounds twice: 1 + 2^-24 + 2^-60 lies
    above the midpoint of 1 and 1 + 2^-23 (fp64 drops the 2^-60 and the tie goes to even, 1)."""
    a, b = np.float32(2.0 ** -30), np.float32(2.0 ** -30)
    c = np.float32(1.0)
    assert R.fma_f32(a, b, c) == np.float32(1.0)
    c = np.float32(1.0 + 2.0 ** -23)           # odd mantissa
    half = np.float32(2.0 ** -24)
    assert R.fma_f32(half, np.float32(1.0), c) == np.float32(1.0 + 2.0 ** -22)      # a tie: to even
    assert R.round_f32(R.Fraction(1) + R.Fraction(1, 2 ** 24) + R.Fraction(1, 2 ** 60)) == np.float32(1.0 + 2.0 ** -23)
    assert np.float32(1.0 + 2.0 ** -24 + 2.0 ** -60) == np.float32(1.0)             # what rounding twice gives
    assert R.fma_f32(np.float32(3.0), np.float32(0.1), np.float32(-0.25)) == np.float32(
        float(R.Fraction(float(np.float32(0.1))) * 3 - R.Fraction(1, 4)))


@pytest.mark.parametrize("count", [2, 3, 5, 7, 13, 17, 33, 36, 37, 64])
@pytest.mark.parametrize("rng", [(0.0, math.pi), (0.0, 2 * math.pi), (0.2, 1.7), (-1.0, 2.5), (2.5, -1.0)])
def test_angles_against_linspace(count, rng):
    """Within one ulp of the range's larger end of np.linspace in fp64; the ends themselves exact
    at the start and within that ulp at the end."""
    a = R.bake_angles(count, *rng)
    ref = np.linspace(float(np.float32(rng[0])), float(np.float32(rng[1])), count)
    ulp = float(np.spacing(np.float32(max(abs(rng[0]), abs(rng[1])))))
    assert a.dtype == np.float32 and a[0] == np.float32(rng[0])
    assert np.abs(a.astype(np.float64) - ref).max() <= ulp


def test_single_row_and_single_column():
    """h == 1 and w == 1: the step is 0 and the one angle is the range's start."""
    assert R.bake_angles(1, 0.3, 2.0).tolist() == [np.float32(0.3)]
    d, th, ph = R.bake_directions(5, 1, (0.7, 1.9), (0.0, 1.0))
    assert d.shape == (5, 3) and th.tolist() == [np.float32(0.7)] and len(set(d[:, 2].tolist())) == 1
    d, th, ph = R.bake_directions(1, 5, (0.7, 1.9), (0.4, 1.0))
    assert ph.tolist() == [np.float32(0.4)]
    np.testing.assert_allclose(np.arctan2(d[:, 1], d[:, 0]), 0.4, atol=1e-6)
    d, _, _ = R.bake_directions(1, 1)
    assert d.tolist() == [[0.0, 0.0, 1.0]]


def test_directions_are_pixel_major_and_unit():
    d, th, ph = R.bake_directions(7, 5)
    assert d.shape == (35, 3) and d.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=3e-7)
    x, y = 3, 2
    want = [math.cos(float(ph[x])) * math.sin(float(th[y])), math.sin(float(ph[x])) * math.sin(float(th[y])), math.cos(float(th[y]))]
    np.testing.assert_allclose(d[y * 7 + x], want, atol=1e-7)


@VF
def test_reversed_window_is_the_mirrored_window(variant, frame):
    """check_bake allows theta1 < theta0 and phi1 < phi0: the angles are the forward window's in
    reverse order within 2 ulp of the range's larger end (the step is rounded once, and carried
    count - 1 times from the other end), and the fp64 oracle's image is the mirrored one within
    the two references' bounds."""
    lam = list(R.bake_lists(variant).values())[0]
    w, h = R.WINDOW["size"]
    fwd = R.BakeReference(variant, frame, w, h, R.WINDOW["theta"], R.WINDOW["phi"], lam)
    rev = R.BakeReference(variant, frame, w, h, R.WINDOW_REVERSED["theta"], R.WINDOW_REVERSED["phi"], lam)
    assert np.abs(rev.theta[::-1].astype(np.float64) - fwd.theta).max() <= 2 * float(np.spacing(np.float32(1.7)))
    assert np.abs(rev.phi[::-1].astype(np.float64) - fwd.phi).max() <= 2 * float(np.spacing(np.float32(2.5)))
    mirror = lambda a: a.reshape(-1, h, w)[:, ::-1, ::-1].reshape(a.shape)   # noqa: E731
    assert (np.abs(mirror(rev.o64) - fwd.o64) <= fwd.bound + mirror(rev.bound)).all()
    assert not fwd.loose.any() and not rev.loose.any()


# ---------------------------------------------------------------- the oracle alone
@VF
def test_fp32_oracle_meets_the_bound_and_the_caps(variant, frame):
    """The fp32 oracle as the image: inside the bound on every pixel of every image (trivially so
    by the |o32 - o64| term; its ratio is what a bake is measured next to), no loose pixel outside
    the sun windows and at most 3 % inside them, and pixels structurally below the horizon in
    every image that has rows there."""
    for lname, lam in R.bake_lists(variant).items():
        for image, w, h, theta, phi, cap in R.bake_images(frame):
            ref = R.BakeReference(variant, frame, w, h, theta, phi, lam)
            worst, nloose = ref.check(ref.o32, cap, f"ORACLE32 | {variant} {frame} {lname} {image}")
            assert worst <= 1.0
            if image.startswith("sun"):
                assert 0 < nloose <= 0.03 * w * h and (ref.o64.max(axis=0) > 100 * np.median(ref.o64.max(axis=0))).any()
            if image.startswith("sphere") and h >= 5:
                assert ref.dark.any() and not ref.dark.all()
            assert np.isfinite(ref.bound).all() and (ref.bound > 0).all()


@VF
def test_a_bake_one_column_off_misses_the_bound(variant, frame):
    """What the bound can see: the fp64 image with column x + 1 in place of column x is over the
    bound on many pixels, from (9, 7) up; so is an image with one lit pixel below the horizon."""
    lam = list(R.bake_lists(variant).values())[-1]
    for w, h in ((9, 7), (37, 13), (64, 33)):
        ref = R.BakeReference(variant, frame, w, h, lam=lam)
        shifted = np.roll(ref.o64.reshape(-1, h, w), -1, axis=2).reshape(ref.o64.shape)
        over = (ref.ratio(shifted) > 1.0).any(axis=0)
        assert over.sum() >= 16, (w, h, int(over.sum()))
        with pytest.raises(AssertionError, match="over the bound"):
            ref.check(shifted, 0.0, "shifted")
        lit = ref.o64.copy()
        lit[0, np.flatnonzero(ref.dark)[0]] = 1e-12
        with pytest.raises(AssertionError):
            ref.check(lit, 0.0, "lit")


# ---------------------------------------------------------------- the input generators
@pytest.mark.parametrize("frame", R.FRAMES)
def test_directions_hold_every_kind(frame):
    """Every eighth direction inside the disc, the next in the limb band on both sides of the
    cutoff, the next below the emitter's horizon; a batch of every size of SIZES starts with a
    disc direction."""
    n = 4099
    wo = R.directions(n, frame)
    inf = R.oracles("rgb", frame)[0].info()
    loc = R.to_local(frame, wo).astype(np.float64)
    cosg = loc @ inf["sun_dir_local"]
    assert (cosg[::8] >= math.cos(math.radians(0.21))).all() and R.sun_lanes(frame, wo)[::8].all()
    band = cosg[1::8]
    assert (band > inf["cos_cutoff"]).sum() > 50 and (band < inf["cos_cutoff"]).sum() > 50
    assert (loc[2::8, 2] < 0).all()
    np.testing.assert_allclose(np.linalg.norm(wo.astype(np.float64), axis=1), 1.0, atol=3e-7)
    for m in R.SIZES:
        assert R.sun_lanes(frame, R.directions(m, frame))[0]
    lam = R.lambdas(n)
    assert lam.shape == (16, n) and {300.0, 800.0, 320.0, 720.0} <= set(lam[:, :8].ravel().tolist())


def test_masks():
    for n in R.SIZES:
        assert R.mask("none", n) is None
        for kind in R.MASKS[1:]:
            m = R.mask(kind, n)
            assert m.dtype == np.uint8 and m.shape == (n,)
        assert R.mask("all_on", n).all() and not R.mask("all_off", n).any()
        tail, body = R.mask("tail_off", n), R.mask("body_off", n)
        assert (tail != 0).sum() == n - n % 4 and (body != 0).sum() == n % 4 and not ((tail != 0) & (body != 0)).any()
    assert set(np.unique(R.mask("on_bytes", 4099)).tolist()) == {0, 1, 2, 0x80, 0xFF}


# ---------------------------------------------------------------- refusals without a device
def _refused(rc, text):
    assert rc == 1, rc            # SUNSKY_ERROR_INVALID_VALUE
    assert text in ss.lib().sunsky_last_error(), ss.lib().sunsky_last_error()


def test_eval_and_bake_refusals_on_a_host_only_emitter():
    """The counts and strides parts 1, 3 and 5 of test_gpu_eval_shapes.py show to write nothing on
    the GPU, here by their messages (test_capi_cpu.py has the bake's image size and the
    host-only refusal of the bake)."""
    lib = ss.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    vin = ss._capi.Vec3In(p, p, p)
    lam = (ctypes.c_float * 33)(*([500.0] * 33))
    spec = ss.SunskyEmitter(R.emitter_dict(), "spectral", device="host")
    rgb = ss.SunskyEmitter(R.emitter_dict(), "rgb", device="host")
    for fn in (lib.sunsky_eval, lib.sunsky_eval_direction):
        for nlam in (0, 17, -1):
            _refused(fn(spec._h, vin, p, nlam, 8, None, 8, p, 8, None), b"1..16 wavelength planes")
        _refused(fn(spec._h, vin, None, 4, 8, None, 8, p, 8, None), b"1..16 wavelength planes")
        _refused(fn(spec._h, vin, p, 2, 8, None, 8, p, 7, None), b"out_stride < n")
        _refused(fn(spec._h, vin, p, 2, 7, None, 8, p, 8, None), b"wl_stride < n")
        _refused(fn(rgb._h, vin, None, 0, 0, None, 8, p, 7, None), b"out_stride < n")
        _refused(fn(rgb._h, vin, None, 0, 0, None, 8, None, 8, None), b"null ray / output pointer")
        # a single plane: the strides are not looked at, so the call gets as far as the device
        assert fn(spec._h, vin, p, 1, 0, None, 8, p, 0, None) != 0
        assert b"host-only" in lib.sunsky_last_error()
        assert fn(rgb._h, vin, None, 0, 0, None, 0, p, 0, None) == 0          # an empty batch
    for m in (0, 33, -1):
        _refused(lib.sunsky_eval_spectral_broadcast(spec._h, vin, lam, m, None, 8, p, 8, None), b"1..32 broadcast wavelengths")
    _refused(lib.sunsky_eval_spectral_broadcast(spec._h, vin, None, 4, None, 8, p, 8, None), b"1..32 broadcast wavelengths")
    _refused(lib.sunsky_eval_spectral_broadcast(rgb._h, vin, lam, 4, None, 8, p, 8, None), b"needs a spectral emitter")
    _refused(lib.sunsky_eval_spectral_broadcast(spec._h, vin, lam, 2, None, 8, p, 7, None), b"out_stride < n")
    assert lib.sunsky_eval_spectral_broadcast(spec._h, vin, lam, 1, None, 8, p, 0, None) != 0
    assert b"host-only" in lib.sunsky_last_error()
    for w, h in R.LAYOUT_SIZES:
        _refused(lib.sunsky_bake_latlong(rgb._h, w, h, 0.0, 3.0, 0.0, 6.0, None, 0, buf, w * h - 1, None),
                 b"out_stride < width * height")
        _refused(lib.sunsky_bake_latlong(spec._h, w, h, 0.0, 3.0, 0.0, 6.0, lam, 11, buf, w * h - 1, None),
                 b"out_stride < width * height")
    _refused(lib.sunsky_bake_latlong(spec._h, 8, 5, 0.0, 3.0, 0.0, 6.0, lam, 33, buf, 40, None), b"1..32 wavelengths")
    _refused(lib.sunsky_bake_latlong(spec._h, 8, 5, 0.0, 3.0, 0.0, 6.0, lam, 0, buf, 40, None), b"1..32 wavelengths")
    _refused(lib.sunsky_bake_latlong(rgb._h, 8, 5, 0.0, 3.0, 0.0, 6.0, lam, 3, buf, 40, None), b"RGB bake takes no wavelengths")
    _refused(lib.sunsky_bake_latlong(rgb._h, 8, 5, 0.0, 3.0, 0.0, 6.0, None, 0, None, 40, None), b"null output pointer")
    # a reversed window is a valid request: it gets as far as the device
    assert lib.sunsky_bake_latlong(rgb._h, 8, 5, 1.7, 0.2, 2.5, -1.0, None, 0, buf, 40, None) != 0
    assert b"host-only" in lib.sunsky_last_error()
