"""Sequence sampling without a GPU (sunsky_sequence_prepare_sampling and the read-backs on
host-only sequences): the ABI additions, the table against the oracle's sky luminance, B_k
against the oracle's disc centre, the normalisations, the derived scalars, the refusals, and the
numpy restatement (tests/sequence_sampling_reference.py) as a density."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import sunsky_amd as ss
from sunsky_amd import _capi
from sequence_cases import (DAY_TIMES, DAY_TURBIDITY, DAY_WEIGHTS, TURBIDITY, WEIGHTS, base_dict, batch_wo, frame_dict,
                            frame_dirs)
from sequence_sampling_reference import NODE_LAMBDAS, SamplingReference, cell_centres, luminance

NEW_SYMBOLS = ["sunsky_sequence_prepare_sampling", "sunsky_sequence_sampling_info", "sunsky_sequence_get_sampling_table",
               "sunsky_sequence_sample_direction", "sunsky_sequence_pdf_direction"]
VARIANTS = ["rgb", "spectral"]
TABLES = [(8, 16), (16, 32), (64, 256)]
EPS = 2.0 ** -24


def test_library_exports_the_sampling_abi():
    L = C.CDLL(ss.LIB_PATH)
    declared = ss.declared_functions()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert name in _capi._SIGS, name
    assert ss.lib().sunsky_abi_version() == 7
    for name in ("prepare_sampling", "sampling_info", "sampling_table", "sample_direction", "pdf_direction"):
        assert hasattr(ss.SunskySequence, name)


@functools.lru_cache(maxsize=None)
def host_case(variant, frames="five", **kw):
    base = base_dict(**kw)
    parent = ss.SunskyEmitter(base, variant=variant, device="host")
    if frames == "five":
        dirs, turb, wts = frame_dirs(), TURBIDITY, WEIGHTS
    elif frames == "day":
        dirs = np.stack([ss.sun_coordinates(*t) for t in DAY_TIMES]).astype(np.float32)
        turb, wts = DAY_TURBIDITY, DAY_WEIGHTS
    else:   # K = 1
        dirs, turb, wts = frame_dirs()[1:2], TURBIDITY[1:2], [1.0]
    return base, parent, ss.SunskySequence(parent, dirs, turb, wts), dirs, turb, wts


def oracle_frame_luminance(base, dirs, turb, variant, wo, **scales):
    """(K, n) fp32-oracle luminance of every frame's single emitter at local directions wo."""
    spectral = variant == "spectral"
    lam = np.repeat(np.asarray(NODE_LAMBDAS, np.float32)[:, None], wo.shape[0], 1) if spectral else None
    out = []
    for k in range(len(turb)):
        o = O.Oracle(dict(frame_dict(base, dirs[k], turb[k]), **scales), variant, "jit", "f32")
        v = o.eval(-wo.astype(np.float32), lam)
        out.append(luminance(v.T if spectral else v, spectral))
    return np.array(out)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size", TABLES)
def test_table_equals_the_oracles_sky_luminance_at_the_cell_centres(variant, size):
    """f_ij against sum_k w_k Y(sky_k(centre)) of sun_scale-0 oracle emitters, at the accumulation
    bar of tests/test_gpu_sequence.py: 1e-5 max f + (K + 2) 2^-24 sum_k w_k |v_k|."""
    base, _, seq, dirs, turb, wts = host_case(variant)
    seq.prepare_sampling(*size)
    f = seq.sampling_table("sky")
    assert f.shape == size and seq.sampling_info()["n_z"] == size[0] and seq.sampling_info()["n_phi"] == size[1]
    v = oracle_frame_luminance(base, dirs, turb, variant, cell_centres(*size), sun_scale=0.0)
    w = np.asarray(wts, np.float64)[:, None]
    ref, mag = (w * v).sum(0), (w * np.abs(v)).sum(0)
    bound = 1e-5 * f.max() + (len(turb) + 2) * EPS * mag
    err = np.abs(f.reshape(-1).astype(np.float64) - ref)
    print(f"{variant} {size}: worst {np.max(err / bound):.3f} x bound, max f {f.max():.4g}")
    assert np.all(f >= 0) and f.max() > 0
    assert np.all(err <= bound), (np.max(err / bound), int((err > bound).sum()))


@pytest.mark.parametrize("variant", VARIANTS)
def test_suns_equal_the_disc_centre_luminance(variant):
    """B_k within 1e-5 of Y of a single emitter's disc-centre value with sky_scale 0 (the fp32
    oracle stands in for the host emitter, which has no eval); 0 for the night frame."""
    base, _, seq, dirs, turb, _ = host_case(variant)
    seq.prepare_sampling(8, 16)
    B = seq.sampling_table("B")
    for k in range(len(turb)):
        s = seq.frame(k)["sun_dir_local"]
        ref = oracle_frame_luminance(base, dirs[k:k + 1], turb[k:k + 1], variant, s[None, :].astype(np.float64),
                                     sky_scale=0.0)[0, 0]
        print(f"frame {k}: B {B[k]:.6g}, oracle {ref:.6g}")
        if s[2] < 0:
            assert B[k] == 0
        else:
            assert ref > 0 and abs(B[k] - ref) <= 1e-5 * ref
    assert any(seq.frame(k)["sun_dir_local"][2] < 0 for k in range(len(turb)))


@pytest.mark.parametrize("frames", ["five", "day", "one"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_normalisation_and_derived_scalars(variant, frames):
    _, parent, seq, _, _, wts = host_case(variant, frames)
    seq.prepare_sampling(16, 32)
    r = SamplingReference(seq, parent.info()["cos_cutoff"])
    assert abs(float(r.q.astype(np.float64).sum()) - 1.0) <= 1e-6
    for cdf in [r.row_cdf, r.frame_cdf] + list(r.cell_cdf):
        assert np.all(np.diff(cdf) >= 0) and cdf[-1] == 1.0 and cdf[0] >= 0
    wB = np.asarray(wts, np.float64) * r.B
    np.testing.assert_allclose(r.q, wB / wB.sum(), rtol=0, atol=1e-6)
    assert np.all(r.q[np.asarray(wts) == 0] == 0)
    # the CDFs are those of the read-back values
    np.testing.assert_allclose(r.row_cdf, np.cumsum(r.f.astype(np.float64).sum(1)) / r.S, rtol=0, atol=1e-6)
    np.testing.assert_allclose(r.frame_cdf, np.cumsum(wB) / wB.sum(), rtol=0, atol=1e-6)
    rows = r.f.astype(np.float64)
    np.testing.assert_allclose(r.cell_cdf, np.cumsum(rows, 1) / rows.sum(1, keepdims=True), rtol=0, atol=1e-6)
    M, P, w = r.masses()
    i = seq.sampling_info()
    assert abs(i["w_sky"] - w) <= 1e-6 and 0 < w < 1
    assert abs(i["sky_mass"] - M) <= 1e-6 * M and abs(i["sun_mass"] - P) <= 1e-6 * P


@pytest.mark.parametrize("variant", VARIANTS)
def test_sky_only_and_sun_only(variant):
    _, _, seq, _, _, _ = host_case(variant, sun_scale=0.0)
    seq.prepare_sampling(8, 16)
    assert seq.sampling_info()["w_sky"] == 1.0 and np.all(seq.sampling_table("q") == 0)
    _, _, seq, _, _, _ = host_case(variant, sky_scale=0.0)
    seq.prepare_sampling(8, 16)
    assert seq.sampling_info()["w_sky"] == 0.0 and np.all(seq.sampling_table("sky") == 0)


def test_a_dark_sequence_is_refused():
    parent = ss.SunskyEmitter(base_dict(), device="host")
    night = frame_dirs()[4:5]
    seq = ss.SunskySequence(parent, np.concatenate([night, night]), [3.0, 5.0], [1.0, 2.0])
    with pytest.raises(ValueError, match="the sequence is dark"):
        seq.prepare_sampling()
    seq = ss.SunskySequence(parent, frame_dirs()[:2], weights=[0.0, 0.0])   # every weight 0
    with pytest.raises(ValueError, match="the sequence is dark"):
        seq.prepare_sampling(8, 16)
    assert ss.lib().sunsky_sequence_prepare_sampling(seq._h, 8, 16) == 1   # SUNSKY_ERROR_INVALID_VALUE


@pytest.mark.parametrize("variant", VARIANTS)
def test_validation(variant):
    parent = ss.SunskyEmitter(base_dict(), variant=variant, device="host")
    seq = ss.SunskySequence(parent, frame_dirs(), TURBIDITY, WEIGHTS)
    for size in [(0, 16), (1025, 16), (8, 3), (8, 4097), (1024, 2048)]:
        with pytest.raises(ValueError, match="sampling table size out of range"):
            seq.prepare_sampling(*size)
    lam = [550.0] if variant == "spectral" else None
    # before prepare_sampling: every sampling call names the missing call
    for call in (seq.sampling_info, lambda: seq.sampling_table("sky"),
                 lambda: seq.sample_direction(None, np.zeros((2, 4), np.float32), wavelengths=lam),
                 lambda: seq.pdf_direction(None, np.zeros((3, 4), np.float32))):
        with pytest.raises(ValueError, match="sunsky_sequence_prepare_sampling first"):
            call()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    v3, o3 = _capi.Vec3In(p, p, p), _capi.Vec3Out(p, p, p)
    none_in, none_out = _capi.Vec3In(None, None, None), _capi.Vec3Out(None, None, None)
    lam_p, m = ((C.c_float * 1)(550.0), 1) if variant == "spectral" else (None, 0)
    L = ss.lib()

    def sample():
        return L.sunsky_sequence_sample_direction(seq._h, p, p, none_in, lam_p, m, None, 4, o3, p, None, none_out, p, 4, None)

    assert sample() == 1 and b"sunsky_sequence_prepare_sampling first" in L.sunsky_last_error()
    assert L.sunsky_sequence_pdf_direction(seq._h, v3, None, 4, p, None) == 1
    assert b"sunsky_sequence_prepare_sampling first" in L.sunsky_last_error()
    # after it: a host-only sequence still launches nothing (the pointers are never read)
    seq.prepare_sampling(1, 4)
    seq.prepare_sampling(1024, 4)   # the limits themselves are valid; a second call replaces the tables
    seq.prepare_sampling(1, 4096)
    seq.prepare_sampling(8, 16)
    assert seq.sampling_table("cell_cdf").shape == (8, 16)
    assert sample() == 1 and b"host-only sequence" in L.sunsky_last_error()
    assert L.sunsky_sequence_pdf_direction(seq._h, v3, None, 4, p, None) == 1
    assert b"host-only sequence" in L.sunsky_last_error()
    with pytest.raises(ValueError, match="host-only"):
        seq.pdf_direction(None, np.zeros((3, 4), np.float32))
    # argument validation of the batch call, as the existing sequence entry points'
    if variant == "spectral":
        assert L.sunsky_sequence_sample_direction(seq._h, p, p, none_in, None, 0, None, 4, o3, p, None, none_out, p, 4, None) == 1
        assert b"broadcast wavelengths" in L.sunsky_last_error()
    else:
        one = (C.c_float * 1)(550.0)
        assert L.sunsky_sequence_sample_direction(seq._h, p, p, none_in, one, 1, None, 4, o3, p, None, none_out, p, 4, None) == 1
        assert b"takes no wavelengths" in L.sunsky_last_error()
        assert L.sunsky_sequence_sample_direction(seq._h, p, p, none_in, None, 0, None, 4, o3, p, None, none_out, p, 3, None) == 1
        assert b"weight_stride" in L.sunsky_last_error()
    assert L.sunsky_sequence_sample_direction(seq._h, None, p, none_in, lam_p, m, None, 4, o3, p, None, none_out, p, 4, None) == 1
    assert L.sunsky_sequence_get_sampling_table(seq._h, 9, None, 0, None) == 1
    assert L.sunsky_sequence_sample_direction(seq._h, None, None, none_in, lam_p, m, None, 0, none_out, None, None, none_out,
                                              None, 0, None) == 0   # an empty batch


@pytest.mark.parametrize("size", TABLES)
def test_the_restatement_is_a_density(size):
    """sum over cells of f / (S omega) omega = 1, so the sky part integrates to w_sky; the sun
    part analytically: each cone has solid angle 2 pi (1 - cos_cutoff) = 1 / sun_pdf and sum q = 1.
    The reference's own pdf() gives exactly that at cell centres and cone axes, and the boundary
    lanes it leaves out of tests/sequence_cases.batch_wo stay under the GPU test's 0.5 % cap."""
    _, parent, seq, _, _, _ = host_case("rgb")
    seq.prepare_sampling(*size)
    inf = parent.info()
    r = SamplingReference(seq, inf["cos_cutoff"])
    w = float(r.w_sky)
    centres = cell_centres(*size)
    hit, _ = r.cone_hits(centres)
    p, _ = r.pdf(centres)
    sky_part = p - (1 - w) * float(r.sun_pdf) * (hit * r.q[None, :].astype(np.float64)).sum(1)
    assert abs(sky_part.sum() * r.omega - w) <= 1e-6
    cone = 2 * np.pi * (1.0 - float(r.cos_cutoff))
    assert abs(float(r.sun_pdf) * cone - 1.0) <= 1e-5   # fp32 1 - cos_cutoff
    assert abs((1 - w) * float(r.sun_pdf) * cone * float(r.q.astype(np.float64).sum()) - (1 - w)) <= 2e-5
    # at a cone axis the sun term is that frame's q (plus any overlapping cone)
    for k in np.nonzero(r.q > 0)[0]:
        pk, _ = r.pdf(r.suns[k:k + 1])
        row, col, _ = r.cells(r.suns[k:k + 1])
        own = w * float(r.f[row[0], col[0]]) / (r.S * r.omega) + (1 - w) * float(r.sun_pdf) * float(r.q[k])
        assert pk[0] >= own * (1 - 1e-12)
    wo = batch_wo(list(r.suns), inf["sun_half_aperture"])
    _, leave = r.pdf(wo)
    print(f"{size}: {leave.mean():.2e} of batch_wo left out")
    assert leave.mean() <= 0.005
