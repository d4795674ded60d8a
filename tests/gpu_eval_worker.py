"""The calls both sides of tests/test_gpu_eval_shapes.py and tools/eval_shapes_measure.py make: the
eval entry points (sunsky_eval, sunsky_eval_direction, sunsky_eval_spectral_broadcast) and
sunsky_bake_latlong through ss.lib(), every plane in an allocation of its own so that each base,
each stride and the mask's alignment is set on its own (Layout), the outputs canaried (Buf: 64
guard floats at either end, every pad column and one plane the call does not use).

The baseline layout is what selects the 4-directions-per-lane kernels (sunsky_launch.cpp
vec4_count): every plane base 16-byte aligned, the strides n rounded up to 4 floats, the mask
4-byte aligned -- a v4 body of n & ~3 directions plus a v1 tail."""
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
import eval_shapes_reference as R  # noqa: E402
from gpu_direct_worker import CANARY, PAD  # noqa: E402

GUARD = 64
INVALID_VALUE = 1      # SUNSKY_ERROR_INVALID_VALUE
PLANES = ("x", "y", "z", "out", "lam")


def emitter(variant, precision, frame="identity"):
    return ss.SunskyEmitter(R.emitter_dict(frame), variant, precision=precision)


def up4(n):
    return (n + 3) & ~3


class Layout:
    """Where a call's planes lie.  off: the planes (of PLANES) based one float off 16-byte alignment;
    mask_off: the mask one byte off 4-byte alignment; ostride / lstride: the row strides (None: n
    rounded up to 4 floats)."""

    def __init__(self, off=(), mask_off=False, ostride=None, lstride=None, name=None):
        self.off, self.mask_off, self.ostride, self.lstride = frozenset(off), mask_off, ostride, lstride
        self.name = name or "+".join(sorted(self.off) + (["mask"] if mask_off else []) +
                                     [f"{k}={v}" for k, v in (("ostride", ostride), ("lstride", lstride)) if v is not None]) or "baseline"


def layouts(n):
    """The baseline and every variant of it that changes one condition of vec4_count, then all."""
    out = [Layout()] + [Layout(off=(p,)) for p in PLANES]
    out += [Layout(mask_off=True), Layout(ostride=n + PAD), Layout(lstride=n + PAD),
            Layout(off=PLANES, mask_off=True, ostride=n + PAD, lstride=n + PAD, name="all")]
    return out


class Buf:
    """rows planes of n fp32 at a row stride, the first based GUARD (+ 1 when off) floats into a
    16-byte aligned allocation that ends with GUARD more; every element holds CANARY (an output)
    or src's rows (an input).  stride 0 (allowed for a single plane) lays one plane."""

    def __init__(self, rows, n, stride, off=False, src=None):
        self.rows, self.n, self.stride = rows, n, stride
        self.base = GUARD + (1 if off else 0)
        size = self.base + max(rows - 1, 0) * stride + up4(n) + GUARD
        self.raw = torch.full((size,), CANARY, dtype=torch.int32, device="cuda")
        self.buf = self.raw.view(torch.float32)
        assert self.raw.data_ptr() % 16 == 0 and (self.ptr() % 16 != 0) == bool(off)
        if src is not None:
            for r in range(rows):
                self.row(r)[:] = src[r]
        self.written = torch.zeros(size, dtype=torch.bool, device="cuda")

    def row(self, r):
        return self.buf[self.base + r * self.stride:self.base + r * self.stride + self.n]

    def ptr(self, r=0):
        return self.buf.data_ptr() + 4 * (self.base + r * self.stride)

    def columns(self, rows):
        """Columns [0, n) of the first `rows` planes: what a call may write -> (rows, n) numpy."""
        for r in range(rows):
            self.written[self.base + r * self.stride:self.base + r * self.stride + self.n] = True
        if not rows:
            return np.zeros((0, self.n), np.float32)
        return torch.stack([self.row(r) for r in range(rows)]).cpu().numpy()

    def untouched(self):
        """Elements outside every columns() taken so far that no longer hold the canary."""
        return int(((self.raw != CANARY) & ~self.written).sum())


def mask_plane(m, off=False):
    """The uint8 mask on the GPU, its base 4-byte aligned or one byte past that -> (tensor, pointer)."""
    if m is None:
        return None, None
    raw = torch.zeros(16 + len(m) + 16, dtype=torch.uint8, device="cuda")
    b = 16 + (1 if off else 0)
    raw[b:b + len(m)] = torch.from_numpy(np.ascontiguousarray(m, np.uint8)).cuda()
    p = raw.data_ptr() + b
    assert (p % 4 != 0) == bool(off)
    return raw, p


def eval_call(em, entry, wo, lam=None, nlam=0, mask=None, lay=None, expect=None, spare=1):
    """One call of entry ("eval": wi = -wo, "eval_direction": d = wo, "broadcast": wi = -wo with lam a
    host list) -> (columns [0, n) of the planes the call writes as (rows, n) numpy, canary
    elements lost).  wo (3, n) numpy; lam (16, n) numpy planes of which the first nlam are passed
    (per-ray entries), or the broadcast list.  expect: the status the call must return instead
    of OK; nothing may be written then.  spare: planes allocated past the ones in use."""
    lay = lay or Layout()
    lib, h, st = ss.lib(), em._h, em._stream()
    n = wo.shape[1]
    d = torch.from_numpy(np.ascontiguousarray(wo if entry == "eval_direction" else -wo)).cuda()
    xyz = [Buf(1, n, up4(n), p in lay.off, d[i:i + 1]) for i, p in enumerate("xyz")]
    vin = ss._capi.Vec3In(*[b.ptr() for b in xyz])
    keep, mptr = mask_plane(mask, lay.mask_off)
    ostride = up4(n) if lay.ostride is None else lay.ostride
    if entry == "broadcast":
        m = len(lam)
        rows = min(max(m, 0), R.MAX_BROADCAST) if expect is None else 1
        out = Buf(rows + spare if ostride >= n else rows, n, ostride, "out" in lay.off)
        arr = (ctypes.c_float * max(m, 1))(*[float(v) for v in lam])
        rc = lib.sunsky_eval_spectral_broadcast(h, vin, arr, m, mptr, n, out.ptr(), ostride, st)
    else:
        spec = em.is_spectral
        rows = (nlam if spec else 3) if expect is None else 1
        lstride = up4(n) if lay.lstride is None else lay.lstride
        lrows = min(max(nlam, 1), R.MAX_LAMBDA)
        lb = Buf(lrows, n, lstride, "lam" in lay.off, torch.from_numpy(lam[:lrows]).cuda()) if spec else None
        out = Buf(rows + spare if ostride >= n else rows, n, ostride, "out" in lay.off)
        fn = lib.sunsky_eval if entry == "eval" else lib.sunsky_eval_direction
        rc = fn(h, vin, lb.ptr() if spec else None, nlam if spec else 0, lstride if spec else 0, mptr, n, out.ptr(),
                ostride, st)
    torch.cuda.synchronize()
    if expect is None:
        ss._capi.check(rc)
    else:
        assert rc == expect, (rc, expect)
        rows = 0
    return out.columns(rows), out.untouched()


def entries(variant):
    """The calls of the stride, alignment and mask tests -> [(name, entry, kwargs)]."""
    if variant == "rgb":
        return [("eval", "eval", {}), ("eval_direction", "eval_direction", {})]
    out = [(f"{e}_nlam{k}", e, dict(nlam=k)) for e in ("eval", "eval_direction") for k in (1, 3, 4, 5)]
    return out + [("broadcast_m1", "broadcast", dict(lam=[555.0])), ("broadcast_off_nodes", "broadcast", dict(lam=R.OFF_NODES)),
                  ("broadcast_nodes", "broadcast", dict(lam=R.NODES))]


def run_entry(em, entry, kw, inp, mask=None, lay=None, **more):
    """eval_call of one of entries() on R.inputs."""
    lam = kw.get("lam", inp["lam"])
    return eval_call(em, entry, inp["wo"], lam, kw.get("nlam", 0), mask, lay, **more)


def bake_call(em, w, h, theta, phi, lam=None, ostride=None, off=False, expect=None):
    """sunsky_bake_latlong through ss.lib() -> ((C, h w) numpy, canary elements lost); ostride None:
    w h rounded up to 4."""
    n = w * h
    ostride = up4(n) if ostride is None else ostride
    rows = len(lam) if em.is_spectral else 3
    out = Buf(rows + 1 if ostride >= n else 1, max(n, 1), max(ostride, 1), off)
    arr = (ctypes.c_float * len(lam))(*[float(v) for v in lam]) if em.is_spectral else None
    rc = ss.lib().sunsky_bake_latlong(em._h, w, h, float(theta[0]), float(theta[1]), float(phi[0]), float(phi[1]), arr,
                                      len(lam) if em.is_spectral else 0, out.ptr(), ostride, em._stream())
    torch.cuda.synchronize()
    if expect is None:
        ss._capi.check(rc)
    else:
        assert rc == expect, (rc, expect)
        rows = 0
    return out.columns(rows), out.untouched()
