"""torch.autograd bridges: the ray direction of eval() (eval_wi) and the per-frame
parameters of a frame sequence (sequence_eval).

eval_wi(em, wi, ...) is em.eval(si) as a differentiable function of wi: the forward value is
the emitter's own eval kernel (FAST or reference, whichever the emitter is set to), the
backward is SunskyEmitter.eval_vjp_dir on the saved wi and the incoming cotangent.

Only wi carries a gradient.  Wavelengths, the mask and the emitter get none: the parameter
gradients (turbidity, albedo, sun_direction) stay with SunskyEmitter.eval_vjp.  The backward
reads the emitter state current when backward() runs, not a snapshot taken at the forward:
do not update the emitter between the two.  The backward is once_differentiable (there are
no second derivatives).

sequence_eval(seq, wi, weights, turbidity, sun_directions, ...) is seq.eval(wi) as a
differentiable function of the frames: the forward writes the given tensors' values into the
sequence (seq.update, host-synchronous) and evaluates it, the backward is seq.eval_vjp.  The
same caveats hold: the backward reads the sequence as it is when backward() runs, so do not
update it (or call sequence_eval on it again) between a forward and its backward.

sequence_irradiance(seq, normals, weights, ...) is seq.irradiance(normals) as a differentiable
function of the receiver normals and the frame weights -- and, under a horizon profile
(horizon=...), of the profile: the backward is seq.irradiance_vjp, with the same caveat.
"""
import torch
from torch.autograd.function import once_differentiable

from .records import SurfaceInteraction3f


class _EvalWi(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wi, em, wavelengths, active):
        wi = wi.detach()
        ctx.em, ctx.wavelengths, ctx.active = em, wavelengths, active
        ctx.save_for_backward(wi)
        return em.eval(SurfaceInteraction3f(wi=wi, wavelengths=wavelengths), active)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        (wi,) = ctx.saved_tensors
        si = SurfaceInteraction3f(wi=wi, wavelengths=ctx.wavelengths)
        return ctx.em.eval_vjp_dir(si, d_out.contiguous(), ctx.active), None, None, None


def eval_wi(em, wi, wavelengths=None, active=None):
    """em.eval(SurfaceInteraction3f(wi, wavelengths), active), differentiable in wi.

    wi: (3, n) float32 tensor on the emitter's device.  Returns (3, n) (RGB) or (k, n)
    (spectral), bit for bit em.eval's value."""
    if not isinstance(wi, torch.Tensor) or wi.dtype != torch.float32 or wi.dim() != 2 or wi.shape[0] != 3:
        raise ValueError("wi must be a float32 tensor of shape (3, n)")
    if isinstance(wavelengths, torch.Tensor):
        wavelengths = wavelengths.detach()
    return _EvalWi.apply(wi, em, wavelengths, active)


class _SequenceEval(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wi, seq, wavelengths, active, weights, turbidity, sun_directions):
        wi = wi.detach()
        ctx.seq, ctx.wavelengths, ctx.active = seq, wavelengths, active
        ctx.save_for_backward(wi)
        ctx.devices = [t.device if t is not None else None for t in (weights, turbidity, sun_directions)]
        if any(ctx.needs_input_grad[4:7]) and not seq.grad_prepared:
            seq.prepare_grad()   # the update below restages the records
        if weights is not None or turbidity is not None or sun_directions is not None:
            seq.update(sun_directions, turbidity, weights)
        return seq.eval(wi, wavelengths, active)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        (wi,) = ctx.saved_tensors
        seq = ctx.seq
        keys = ("weights", "turbidity", "sun_directions")
        need = dict(zip(keys, ctx.needs_input_grad[4:7]))
        k = len(seq)
        grad = {key: torch.zeros((k, 3) if key == "sun_directions" else (k,), dtype=torch.float32, device=seq.device)
                if need[key] else None for key in keys}
        if any(need.values()):
            seq.eval_vjp(wi, d_out.contiguous(), ctx.wavelengths, ctx.active, grad=grad)
        return (None, None, None, None) + tuple(None if grad[key] is None else grad[key].to(dev)
                                                for key, dev in zip(keys, ctx.devices))


class _SequenceIrradiance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normals, seq, active, weights, horizon):
        nrm = normals.detach()
        hz = None if horizon is None else horizon.detach()
        ctx.seq, ctx.active, ctx.has_horizon = seq, active, hz is not None
        ctx.weights_device = weights.device if weights is not None else None
        ctx.save_for_backward(*((nrm,) if hz is None else (nrm, hz)))
        if weights is not None:
            if seq.irradiance_args is None:
                raise ValueError("sequence_irradiance needs seq.prepare_irradiance(...) first: it prepares again "
                                 "with the same arguments after it has updated the weights")
            seq.update(weights=weights)
            n_z, n_phi, lam = seq.irradiance_args
            seq.prepare_irradiance(n_z, n_phi, lam)
        if (ctx.needs_input_grad[0] or ctx.needs_input_grad[3] or ctx.needs_input_grad[4]) and not seq.irradiance_grad_prepared:
            seq.prepare_irradiance_grad()
        return seq.irradiance(nrm, active) if hz is None else seq.irradiance(nrm, active, horizon=hz)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        nrm, hz = ctx.saved_tensors if ctx.has_horizon else (ctx.saved_tensors[0], None)
        seq = ctx.seq
        need_n, need_w, need_h = ctx.needs_input_grad[0], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        grad = {"normals": torch.empty_like(nrm) if need_n else None,
                "weights": torch.zeros(len(seq), dtype=torch.float32, device=seq.device) if need_w else None}
        if hz is not None:
            # a shared profile's gradient is the torch sum of the per-receiver columns (irradiance_vjp)
            grad["horizon"] = torch.empty(hz.shape, dtype=torch.float32, device=seq.device) if need_h else None
        if need_n or need_w or need_h:
            d = d_out if d_out.dim() == 2 and (d_out.shape[1] <= 1 or d_out.stride(1) == 1) else d_out.contiguous()
            seq.irradiance_vjp(nrm, d, ctx.active, grad=grad, horizon=hz)
        gw = grad["weights"]
        return grad["normals"], None, None, None if gw is None else gw.to(ctx.weights_device), grad.get("horizon")


def sequence_irradiance(seq, normals, weights=None, active=None, horizon=None):
    """seq.irradiance(normals, active, horizon=horizon), differentiable in the normals, in the frame
    weights and in the horizon profile.

    normals: (3, n) float32 tensor on the sequence's device.  weights: a (K,) float32 tensor (any
    device; its values are read on the host) or None to leave the sequence's weights as they are.
    horizon: seq.irradiance's argument, a float32 tensor (H,), (H, 1) or (H, n) on the sequence's
    device, or None for the open sky.
    With weights the forward calls seq.update(weights=...) and seq.prepare_irradiance with the
    arguments of the last prepare_irradiance; it returns bit for bit seq.irradiance's value.  The
    backward is seq.irradiance_vjp: gradients for the normals, on the weights' device for the
    weights and, when it requires grad, for the horizon tensor in its own shape (a shared profile:
    the per-receiver gradients summed by torch.sum).  Do not update the sequence between a forward
    and its backward."""
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[0] != 3:
        raise ValueError("normals must be a float32 tensor of shape (3, n)")
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32):
        raise ValueError("weights must be a float32 tensor or None")
    if horizon is not None and (not isinstance(horizon, torch.Tensor) or horizon.dtype != torch.float32):
        raise ValueError("horizon must be a float32 tensor or None")
    return _SequenceIrradiance.apply(normals, seq, active, weights, horizon)


def sequence_eval(seq, wi, weights=None, turbidity=None, sun_directions=None, wavelengths=None, active=None):
    """seq.eval(wi, wavelengths, active), differentiable in the per-frame tensors passed.

    weights (K,), turbidity (K,), sun_directions (K, 3): float32 tensors (any device; their
    values are read on the host) or None to leave that part of the sequence as it is.  The
    forward calls seq.update with them and returns bit for bit seq.eval's value; the backward
    returns gradients for exactly the tensors passed, on each tensor's device.  wi gets none."""
    if not isinstance(wi, torch.Tensor) or wi.dtype != torch.float32 or wi.dim() != 2 or wi.shape[0] != 3:
        raise ValueError("wi must be a float32 tensor of shape (3, n)")
    for name, t in (("weights", weights), ("turbidity", turbidity), ("sun_directions", sun_directions)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
            raise ValueError(f"{name} must be a float32 tensor or None")
    return _SequenceEval.apply(wi, seq, wavelengths, active, weights, turbidity, sun_directions)
