"""torch.autograd bridge for the ray direction of eval().

eval_wi(em, wi, ...) is em.eval(si) as a differentiable function of wi: the forward value is
the emitter's own eval kernel (FAST or reference, whichever the emitter is set to), the
backward is SunskyEmitter.eval_vjp_dir on the saved wi and the incoming cotangent.

Only wi carries a gradient.  Wavelengths, the mask and the emitter get none: the parameter
gradients (turbidity, albedo, sun_direction) stay with SunskyEmitter.eval_vjp.  The backward
reads the emitter state current when backward() runs, not a snapshot taken at the forward:
do not update the emitter between the two.  The backward is once_differentiable (there are
no second derivatives).
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
