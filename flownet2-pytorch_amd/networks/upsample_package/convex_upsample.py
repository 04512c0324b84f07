"""ConvexUpsample: the learned "convex" upsampling of RAFT and its descendants (``upsample_flow`` in RAFT's ``raft.py``) as one
fused layer -- autograd Function + Module over the ``convex_upsample_cuda`` extension (csrc/binding/convex_upsample_cuda.cpp,
csrc/convex_upsample.hip), and ``upsample_flow(flow, mask)`` with RAFT's signature.

    out[n, c, f y + i, f x + j] = sum_k softmax_k(mask[n, k f^2 + i f + j, y, x]) * scale * flow[n, c, y + ky - 1, x + kx - 1]

with k = 3 ky + kx over the 3 x 3 neighbourhood (zero padding): softmax, unfold, weighted sum, permute and reshape of the
PyTorch composition without any of its intermediates.  ``flow`` is float32 with up to four channels, ``mask`` float32, float16
or bfloat16 with 9 f^2 channels, f in {2, 4, 8}; both get gradients, the backward uses no atomics and is bit-reproducible.
Semantics, arithmetic order and bounds are documented in include/flownet2_hip_upsample.h.  Importing this module fails loudly
if the extension has not been built: the HIP kernels are the only implementation.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import convex_upsample_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

MAX_CHANNELS = 4   # FN2U_MAX_CHANNELS (include/flownet2_hip_upsample.h)


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _fake_inputs(flow, mask, factor, op):
    """check_inputs of csrc/binding/convex_upsample_cuda.cpp, as far as shapes and dtypes decide it."""
    refuse(factor in (2, 4, 8), op, ": factor ", factor, " is not 2, 4 or 8")
    refuse(flow.dim() == 4 and mask.dim() == 4, op, ": flow and mask must be 4-D (N, C, H, W)")
    refuse(1 <= flow.shape[1] <= MAX_CHANNELS, op, ": flow has ", flow.shape[1], " channels, 1 .. ", MAX_CHANNELS, " are supported")
    refuse(mask.shape[1] == 9 * factor * factor, op, ": mask has ", mask.shape[1], " channels, expected 9 * factor^2 = ", 9 * factor * factor)
    refuse(mask.shape[0] == flow.shape[0] and mask.shape[2] == flow.shape[2] and mask.shape[3] == flow.shape[3], op, ": mask ",
           tuple(mask.shape), " must have the batch size, height and width of flow ", tuple(flow.shape))
    refuse(flow.dtype == torch.float32, op, ": flow must be float32, got ", flow.dtype,
           " (RAFT upsamples its flow in float under autocast: use .float())")
    refuse(mask.dtype in (torch.float32, torch.float16, torch.bfloat16), op, ": mask must be float32, float16 or bfloat16, got ", mask.dtype)


def _forward_fake(flow, mask, factor, scale):
    _fake_inputs(flow, mask, factor, "fn2::convex_upsample")
    return flow.new_empty((flow.shape[0], flow.shape[1], factor * flow.shape[2], factor * flow.shape[3]))


def _backward_fake(flow, mask, grad_output, factor, scale):
    _fake_inputs(flow, mask, factor, "fn2::convex_upsample_backward")
    return flow.new_empty(flow.shape), mask.new_empty(mask.shape)   # the mask's gradient keeps the mask's dtype


def _setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.upsample_params = tuple(inputs[2:])


def _grad(ctx, grad_output):
    flow, mask = ctx.saved_tensors
    grad_flow, grad_mask = _backward_op(flow, mask, grad_output, *ctx.upsample_params)
    return grad_flow, grad_mask, None, None


_forward_op = fn2_ops.define("convex_upsample", "(Tensor flow, Tensor mask, int factor, float scale) -> Tensor",
                             convex_upsample_cuda.forward_alloc, _forward_fake, _grad, _setup)
_backward_op = fn2_ops.define("convex_upsample_backward",
                              "(Tensor flow, Tensor mask, Tensor grad_output, int factor, float scale) -> (Tensor, Tensor)",
                              convex_upsample_cuda.backward_alloc, _backward_fake)


class ConvexUpsampleFunction(Function):
    """``apply`` goes straight to the autograd node the extension implements in C++ (``convex_upsample_cuda.apply``);
    ``forward`` / ``backward`` are the same two calls for code that drives a Function's static methods itself."""

    @classmethod
    def apply(cls, flow, mask, factor, scale):
        return convex_upsample_cuda.apply(flow, mask, factor, scale)

    @staticmethod
    def forward(ctx, flow, mask, factor, scale):
        ctx.save_for_backward(flow, mask)
        ctx.upsample_params = (factor, scale)
        if torch.compiler.is_compiling():   # Dynamo traces apply() through this method: the operator it can see
            return _forward_op(flow, mask, factor, scale)
        return convex_upsample_cuda.forward_alloc(flow, mask, factor, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        flow, mask = ctx.saved_tensors
        backward_alloc = _backward_op if torch.compiler.is_compiling() else convex_upsample_cuda.backward_alloc
        grad_flow, grad_mask = backward_alloc(flow, mask, grad_output, *ctx.upsample_params)
        return grad_flow, grad_mask, None, None


class ConvexUpsample(nn.Module):
    """``ConvexUpsample(factor=8, scale=None)(flow, mask)`` -> B x C x factor H x factor W; ``scale=None`` means ``float(factor)``:
    a flow in pixels of the coarse grid becomes one in pixels of the fine grid, as in RAFT."""

    def __init__(self, factor=8, scale=None):
        super().__init__()
        self.factor = factor
        self.scale = scale

    def forward(self, flow, mask):
        scale = float(self.factor) if self.scale is None else self.scale
        return ConvexUpsampleFunction.apply(flow, mask, self.factor, scale)

    def extra_repr(self):
        return f"factor={self.factor}, scale={self.scale}"


def upsample_flow(flow, mask):
    """RAFT's ``upsample_flow(flow, mask)``: [N, C, H, W] -> [N, C, f H, f W], the factor f read off ``mask.shape[1] == 9 f^2``."""
    f = {9 * g * g: g for g in (2, 4, 8)}.get(mask.shape[1] if mask.dim() == 4 else -1)
    if f is None:
        raise ValueError(f"upsample_flow: mask of shape {tuple(mask.shape)} does not have 9 f^2 channels with f in (2, 4, 8)")
    return ConvexUpsampleFunction.apply(flow, mask, f, float(f))
