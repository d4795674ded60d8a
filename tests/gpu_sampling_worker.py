"""Worker of tests/test_gpu_sampling_shapes.py, and the calls both sides of its tests make: the four
sampling entry points (sunsky_sample_direction, sunsky_pdf_direction, sunsky_sample_ray,
sunsky_sample_wavelengths) through ss.lib(), with packed planes (what the Python wrappers pass) or
with every row stride n + PAD, every plane base off 16-byte alignment and canaried outputs
(Planes of gpu_direct_worker.py), any wavelength count and any subset of the optional pointers.

As a program (a fresh child process, started with SUNSKY_AMD_BLOCKS_PER_CU=1 so that every grid
is capped at one workgroup per CU):  gpu_sampling_worker.py <n> <n_vec> <output directory>
runs every (variant, precision) of COMBOS and saves each one's outputs (run_grid) to
<variant>_<precision>.npz.  Exit 0 = all saved."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "mitsuba3-sunsky_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sunsky_amd as ss  # noqa: E402
import sampling_shapes_reference as S  # noqa: E402
from gpu_direct_worker import CANARY, PAD, Planes  # noqa: E402,F401

COMBOS = [(v, p) for v in ("rgb", "spectral") for p in ("fast", "reference")]
INVALID_VALUE = 1      # SUNSKY_ERROR_INVALID_VALUE


def emitter(variant, precision, frame="rotated", semantics="jit"):
    em = ss.SunskyEmitter(S.emitter_dict(frame), variant, semantics, precision=precision)
    em.set_scene(*S.BBOX)
    return em


def set_sphere(em, center, radius):
    """set_scene with the bounding sphere itself (sunsky_emitter_set_scene)."""
    c = (ctypes.c_float * 3)(*[float(x) for x in center])
    ss._capi.check(ss.lib().sunsky_emitter_set_scene(em._h, 1, c, float(radius)))
    em._refresh_info()


def sun_dir(em):
    return em.info()["sun_dir_world"]


def inputs(em, n, seed=71):
    return S.inputs(n, em.sky_sampling_w, seed, sun_dir=sun_dir(em))


def cap_step():
    """Samples one grid-stride step of a one-sample-per-lane kernel covers at one workgroup per CU."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 256


def batch_sizes():
    """(n, n_vec): two and a half grid-stride steps at one workgroup per CU, plus 3, of the
    one-sample-per-lane kernels and of pdf_direction's 4-directions-per-lane kernel."""
    step = cap_step()
    return 2 * step + step // 2 + 3, 4 * (2 * step + step // 2) + 3


class Packed:
    """rows x n elements, contiguous (row stride n), as the Python wrappers allocate them; the
    interface of Planes."""

    def __init__(self, rows, n, src=None, dtype=torch.float32):
        self.rows, self.n, self.stride = rows, n, n
        self.body = torch.zeros((rows, n), dtype=dtype, device="cuda")
        if src is not None:
            self.body[:] = src

    def ptr(self, row=0):
        return self.body[row].data_ptr()

    def v3(self, row=0, cls=None):
        return (cls or ss._capi.Vec3In)(self.ptr(row), self.ptr(row + 1), self.ptr(row + 2))

    def columns(self, rows=None):
        return self.body[:self.rows if rows is None else rows]

    def untouched(self):
        return 0


class Pitched(Planes):
    """rows x n elements at a pitch of n rounded up to 4 floats plus 4, the base 16-byte aligned
    (what sunsky_pdf_direction's 4-directions-per-lane kernel needs), 16 guard elements at either
    end; canaried like Planes."""

    def __init__(self, rows, n, src=None):
        self.rows, self.n, self.stride = rows, n, ((n + 3) & ~3) + 4
        size = 16 + rows * self.stride + 16
        self.raw = torch.full((size,), CANARY, dtype=torch.int32, device="cuda")
        self.buf = self.raw.view(torch.float32)
        self.body = self.buf[16:16 + rows * self.stride].view(rows, self.stride)
        assert self.body.data_ptr() % 16 == 0 and self.stride % 4 == 0
        if src is not None:
            self.body[:, :n] = src
        self.written = torch.zeros(size, dtype=torch.bool, device="cuda")

    def columns(self, rows=None):
        rows = self.rows if rows is None else rows
        self.written[16:16 + self.rows * self.stride].view(self.rows, self.stride)[:rows, :self.n] = True
        return self.body[:rows, :self.n]


def _g(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _planes(cls, rows, n, src=None, dtype=torch.float32):
    return cls(rows, n, _g(src, dtype), dtype) if cls is not Pitched else cls(rows, n, _g(src, dtype))


def _mask(cls, n, mask):
    """The mask plane (uint8), based 1 byte into its allocation when strided; None -> (None, None)."""
    if mask is None:
        return None, None
    m = _planes(Planes if cls is Planes else Packed, 1, n, np.asarray(mask, bool)[None], torch.uint8)
    return m, m.ptr()


def _collect(planes, used):
    torch.cuda.synchronize()
    out = {k: p.columns(used[k]).clone() for k, p in planes.items()}
    return out, {k: p.untouched() for k, p in planes.items()}


V3NULL_IN = ss._capi.Vec3In(None, None, None)
V3NULL_OUT = ss._capi.Vec3Out(None, None, None)


def sample_direction(em, inp, nlam=4, mask=None, it_p=False, dist=False, pos=False, strided=False, expect=None,
                     half=None, lam_strided=None):
    """sunsky_sample_direction through ss.lib() -> ({d (3, n), pdf (1, n), w (C, n), dist (1, n), p
    (3, n): the requested ones}, {name: canary elements lost}).  inp: numpy planes of S.inputs (the
    first nlam wavelength rows are passed); mask: numpy bool or None; it_p / dist / pos: pass
    it.p, request ds.dist, request ds.p (none of them and no mask: the LEAN call).  strided: Planes
    (row stride n + PAD, bases off 16-byte alignment, canaried outputs with one unused weight
    row) instead of packed planes.  expect: the status the call must return instead of OK (the
    outputs are returned as they are).  half: "it_p" / "ds_p" passes that vec3 with a null y.
    lam_strided: the wavelength planes' own layout (wl_stride n + PAD or n) where it is to differ
    from the other planes' (weight_stride)."""
    lib, h, st = ss.lib(), em._h, em._stream()
    cls = Planes if strided else Packed
    n = inp["u"].shape[1]
    spec = em.is_spectral
    u = _planes(cls, 2, n, inp["u"])
    lrows = min(max(nlam, 1), S.MAX_LAMBDA)       # an out-of-range count is refused before anything is read
    lam_cls = cls if lam_strided is None else (Planes if lam_strided else Packed)
    lam = _planes(lam_cls, lrows, n, inp["lam"][:lrows]) if spec else None
    p_in = _planes(cls, 3, n, inp["p"]) if it_p else None
    m, mptr = _mask(cls, n, mask)
    nw = nlam if spec else 3
    rows = min(max(nw, 1), S.MAX_LAMBDA)
    planes = {"d": _planes(cls, 3, n), "pdf": _planes(cls, 1, n), "w": _planes(cls, rows + (1 if strided else 0), n)}
    used = {"d": 3, "pdf": 1, "w": rows}
    if dist:
        planes["dist"], used["dist"] = _planes(cls, 1, n), 1
    if pos:
        planes["p"], used["p"] = _planes(cls, 3, n), 3
    pin = p_in.v3() if it_p else V3NULL_IN
    pout = planes["p"].v3(cls=ss._capi.Vec3Out) if pos else V3NULL_OUT
    if half == "it_p":
        pin = ss._capi.Vec3In(p_in.ptr(0), None, p_in.ptr(2))
    elif half == "ds_p":
        pout = ss._capi.Vec3Out(planes["p"].ptr(0), None, planes["p"].ptr(2))
    rc = lib.sunsky_sample_direction(h, u.ptr(0), u.ptr(1), pin, lam.ptr() if spec else None, nlam if spec else 0,
                                     lam.stride if spec else 0, mptr, n, planes["d"].v3(cls=ss._capi.Vec3Out),
                                     planes["pdf"].ptr(), planes["dist"].ptr() if dist else None, pout,
                                     planes["w"].ptr(), planes["w"].stride, st)
    if expect is None:
        ss._capi.check(rc)
    else:
        assert rc == expect, (rc, expect)
        used = {k: 0 for k in used}       # nothing may be written
    return _collect(planes, used)


def pdf_direction(em, inp, mask=None, layout="packed"):
    """sunsky_pdf_direction -> ({pdf (1, n)}, lost).  layout: packed (the wrapper's planes), pitched
    (16-byte aligned planes: the 4-directions-per-lane body plus a one-per-lane tail), misaligned
    (Planes: one per lane throughout).  The directions are inp["wo"]."""
    cls = {"packed": Packed, "pitched": Pitched, "misaligned": Planes}[layout]
    n = inp["wo"].shape[1]
    d = _planes(cls, 3, n, inp["wo"])
    m, mptr = _mask(cls, n, mask)
    planes = {"pdf": _planes(cls, 1, n)}
    if layout == "pitched":
        assert (mptr is None or mptr % 4 == 0) and all(d.ptr(r) % 16 == 0 for r in range(3)) and planes["pdf"].ptr() % 16 == 0
    ss._capi.check(ss.lib().sunsky_pdf_direction(em._h, d.v3(), mptr, n, planes["pdf"].ptr(), em._stream()))
    return _collect(planes, {"pdf": 1})


def sample_ray(em, inp, mask=None, strided=False):
    """sunsky_sample_ray (sample2 = inp["s2"], sample3 = inp["u"], the wavelength sample inp["ws"])
    -> ({o (3, n), d (3, n), lam (4, n), w (3 | 4, n)}, lost).  lam has four rows in RGB too (the
    kernels store zeros there); strided: one more, unused, weight row."""
    cls = Planes if strided else Packed
    n = inp["u"].shape[1]
    s2, s3 = _planes(cls, 2, n, inp["s2"]), _planes(cls, 2, n, inp["u"])
    ws = _planes(cls, 1, n, inp["ws"][None]) if em.is_spectral else None
    m, mptr = _mask(cls, n, mask)
    nw = 4 if em.is_spectral else 3
    planes = {"o": _planes(cls, 3, n), "d": _planes(cls, 3, n), "lam": _planes(cls, 4, n),
              "w": _planes(cls, nw + (1 if strided else 0), n)}
    ss._capi.check(ss.lib().sunsky_sample_ray(
        em._h, ws.ptr() if ws else None, s2.ptr(0), s2.ptr(1), s3.ptr(0), s3.ptr(1), mptr, n,
        planes["o"].v3(cls=ss._capi.Vec3Out), planes["d"].v3(cls=ss._capi.Vec3Out), planes["lam"].ptr(),
        planes["lam"].stride, planes["w"].ptr(), planes["w"].stride, em._stream()))
    return _collect(planes, {"o": 3, "d": 3, "lam": 4, "w": nw})


def sample_wavelengths(em, inp, mask=None, strided=False):
    """sunsky_sample_wavelengths (si.wi = -inp["wo"], the sample inp["ws"]) -> ({lam (4, n), w (3 | 4,
    n)}, lost)."""
    cls = Planes if strided else Packed
    n = inp["wo"].shape[1]
    wi = _planes(cls, 3, n, -inp["wo"])
    ws = _planes(cls, 1, n, inp["ws"][None]) if em.is_spectral else None
    m, mptr = _mask(cls, n, mask)
    nw = 4 if em.is_spectral else 3
    planes = {"lam": _planes(cls, 4, n), "w": _planes(cls, nw + (1 if strided else 0), n)}
    ss._capi.check(ss.lib().sunsky_sample_wavelengths(em._h, wi.v3(), ws.ptr() if ws else None, mptr, n,
                                                     planes["lam"].ptr(), planes["lam"].stride, planes["w"].ptr(),
                                                     planes["w"].stride, em._stream()))
    return _collect(planes, {"lam": 4, "w": nw})


def head(inp, m):
    """The first m samples of every input plane."""
    return {k: np.ascontiguousarray(v[..., :m]) for k, v in inp.items()}


def run_grid(variant, precision, n, n_vec):
    """What the capped-grid test compares -> {name: numpy array}: the masked general
    sample_direction (spectral: at 4 and at 3 wavelengths), the LEAN spectral call at 3 and at 8
    wavelengths, masked sample_ray, masked sample_wavelengths (n samples each) and masked
    pdf_direction on 16-byte aligned planes (n_vec directions)."""
    em = emitter(variant, precision)
    inp = inputs(em, n_vec, seed=91)
    small, mask = head(inp, n), S.mask("mixed", n_vec)
    calls = {}
    for nlam in ((4, 3) if em.is_spectral else (4,)):
        calls[f"direction_masked_nlam{nlam}"] = sample_direction(em, small, nlam, mask[:n], it_p=True, dist=True, pos=True)
    if em.is_spectral:
        for nlam in (3, 8):
            calls[f"direction_lean_nlam{nlam}"] = sample_direction(em, small, nlam)
    calls["ray_masked"] = sample_ray(em, small, mask[:n])
    calls["wavelengths_masked"] = sample_wavelengths(em, small, mask[:n])
    calls["pdf_masked"] = pdf_direction(em, inp, mask, "pitched")
    out = {}
    for name, (planes, lost) in calls.items():
        assert not any(lost.values()), (name, lost)
        out.update({f"{name}_{k}": v.cpu().numpy() for k, v in planes.items()})
    return out


def main():
    n, n_vec, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    torch.cuda.set_device(0)
    for variant, precision in COMBOS:
        np.savez(os.path.join(outdir, f"{variant}_{precision}.npz"), **run_grid(variant, precision, n, n_vec))
    print("worker ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
