"""CorrLookup: the on-demand correlation lookup of RAFT and its descendants (GMA, RAFT-Stereo, CRAFT, SEA-RAFT) -- autograd
Function + Module over the ``corr_lookup_cuda`` extension (csrc/binding/corr_lookup_cuda.cpp, csrc/corr_lookup.hip), and
``AlternateCorrBlock``, the class RAFT's ``raft.py`` builds with ``alternate_corr=True``.

    out[n, i*D + j, y, x] = scale * sum_corners w * <fmap1[n, :, y, x], fmap2[n, :, y0 + j - r + oy, x0 + i - r + ox]>

with (x0, y0) = floor(coords[n, :, y, x]), D = 2 r + 1 and the bilinear weights w of the fractional parts: RAFT's
``CorrBlock`` lookup without the B x HW x H2 W2 all-pairs volume.  ``coords`` (channel 0 = x, 1 = y, in fmap2 pixels) gets no
gradient and must not require one.  float32 only.  Semantics, bounds and the kernels' domains are documented in
include/flownet2_hip_lookup.h.  Importing this module fails loudly if the extension has not been built: the HIP kernels are
the only implementation.
"""
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import corr_lookup_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

MAX_RADIUS = 8   # FN2L_MAX_RADIUS (include/flownet2_hip_lookup.h)


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _fake_inputs(fmap1, fmap2, coords, radius, op):
    """check_inputs of csrc/binding/corr_lookup_cuda.cpp, as far as shapes and dtypes decide it."""
    refuse(fmap2.dtype == fmap1.dtype and coords.dtype == fmap1.dtype, op, ": fmap2 and coords must have the dtype of fmap1, ", fmap1.dtype)
    refuse(fmap1.dtype == torch.float32, op, ": float32 tensors expected, got ", fmap1.dtype,
           " (RAFT calls its lookup in float under autocast: use .float())")
    refuse(fmap1.dim() == 4 and fmap2.dim() == 4 and coords.dim() == 4, op, ": fmap1, fmap2 and coords must be 4-D (N, C, H, W)")
    refuse(fmap2.shape[0] == fmap1.shape[0] and fmap2.shape[1] == fmap1.shape[1], op, ": fmap2 ", tuple(fmap2.shape),
           " must have the batch and channel counts of fmap1 ", tuple(fmap1.shape))
    refuse(coords.shape[0] == fmap1.shape[0] and coords.shape[1] == 2 and coords.shape[2] == fmap1.shape[2] and coords.shape[3] == fmap1.shape[3],
           op, ": coords has shape ", tuple(coords.shape), ", expected [", fmap1.shape[0], ", 2, ", fmap1.shape[2], ", ", fmap1.shape[3], "]")
    refuse(0 <= radius <= MAX_RADIUS, op, ": radius ", radius, " outside 0 .. ", MAX_RADIUS)


def _forward_fake(fmap1, fmap2, coords, radius, scale):
    _fake_inputs(fmap1, fmap2, coords, radius, "fn2::corr_lookup")
    return fmap1.new_empty((fmap1.shape[0], (2 * radius + 1) ** 2, fmap1.shape[2], fmap1.shape[3]))


def _backward_fake(fmap1, fmap2, coords, grad_output, radius, scale):
    _fake_inputs(fmap1, fmap2, coords, radius, "fn2::corr_lookup_backward")
    return fmap1.new_empty(fmap1.shape), fmap2.new_empty(fmap2.shape)


def _no_coords_gradient(wanted):
    # a silent None for coords would train wrongly: RAFT detaches coords in every iteration, and so must the caller
    if wanted:
        raise RuntimeError("CorrLookup: coords requires grad, but this layer has no gradient for coords (as RAFT's alt_cuda_corr): "
                           "pass coords.detach()")


def _setup(ctx, inputs, output):
    _no_coords_gradient(ctx.needs_input_grad[2])
    ctx.save_for_backward(*inputs[:3])
    ctx.lookup_params = tuple(inputs[3:])


def _grad(ctx, grad_output):
    fmap1, fmap2, coords = ctx.saved_tensors
    grad_fmap1, grad_fmap2 = _backward_op(fmap1, fmap2, coords, grad_output, *ctx.lookup_params)
    return grad_fmap1, grad_fmap2, None, None, None


_forward_op = fn2_ops.define("corr_lookup", "(Tensor fmap1, Tensor fmap2, Tensor coords, int radius, float scale) -> Tensor",
                             corr_lookup_cuda.forward_alloc, _forward_fake, _grad, _setup)
# (backward_alloc raises or warns under torch.use_deterministic_algorithms when the operator runs, as in eager)
_backward_op = fn2_ops.define("corr_lookup_backward",
                              "(Tensor fmap1, Tensor fmap2, Tensor coords, Tensor grad_output, int radius, float scale) -> (Tensor, Tensor)",
                              corr_lookup_cuda.backward_alloc, _backward_fake)


class CorrLookupFunction(Function):
    """``apply`` goes straight to the autograd node the extension implements in C++ (``corr_lookup_cuda.apply``); ``forward`` /
    ``backward`` are the same two calls for code that drives a Function's static methods itself -- through the ``fn2`` operators
    while ``torch.compile`` traces, which is how it sees ``apply``."""

    @classmethod
    def apply(cls, fmap1, fmap2, coords, radius, scale):
        return corr_lookup_cuda.apply(fmap1, fmap2, coords, radius, scale)

    @staticmethod
    def forward(ctx, fmap1, fmap2, coords, radius, scale):
        ctx.save_for_backward(fmap1, fmap2, coords)
        ctx.lookup_params = (radius, scale)
        if torch.compiler.is_compiling():
            _no_coords_gradient(ctx.needs_input_grad[2])
            return _forward_op(fmap1, fmap2, coords, radius, scale)
        return corr_lookup_cuda.forward_alloc(fmap1, fmap2, coords, radius, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        fmap1, fmap2, coords = ctx.saved_tensors
        if torch.compiler.is_compiling():
            grad_fmap1, grad_fmap2 = _backward_op(fmap1, fmap2, coords, grad_output, *ctx.lookup_params)
        else:
            grad_fmap1, grad_fmap2 = corr_lookup_cuda.backward_alloc(fmap1, fmap2, coords, grad_output, *ctx.lookup_params)
        return grad_fmap1, grad_fmap2, None, None, None


class CorrLookup(nn.Module):
    """``CorrLookup(radius, scale=None)(fmap1, fmap2, coords)`` -> B x (2 radius + 1)^2 x H x W; ``scale=None`` means C ** -0.5."""

    def __init__(self, radius, scale=None):
        super().__init__()
        self.radius = radius
        self.scale = scale

    def forward(self, fmap1, fmap2, coords):
        scale = float(fmap1.shape[1]) ** -0.5 if self.scale is None else self.scale
        return CorrLookupFunction.apply(fmap1, fmap2, coords, self.radius, scale)

    def extra_repr(self):
        return f"radius={self.radius}, scale={self.scale}"


class AlternateCorrBlock:
    """The constructor and call of RAFT's ``AlternateCorrBlock`` (``core/corr.py``; ``raft.py`` with ``alternate_corr=True``):
    fmap2 is average-pooled once per level, level i is looked up at ``coords / 2**i`` with scale C ** -0.5, and the levels are
    concatenated along the channels: B x (num_levels * (2 radius + 1)^2) x H x W.  ``coords`` is used detached, as RAFT passes it."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels = num_levels
        self.radius = radius
        self.fmap1 = fmap1.float()
        self.pyramid = [fmap2.float()]
        for _ in range(num_levels - 1):
            self.pyramid.append(F.avg_pool2d(self.pyramid[-1], 2, stride=2))
        self.lookup = CorrLookup(radius)

    def __call__(self, coords):
        coords = coords.detach().float()
        out = [self.lookup(self.fmap1, f2, coords / 2 ** i) for i, f2 in enumerate(self.pyramid)]
        return torch.cat(out, dim=1)
