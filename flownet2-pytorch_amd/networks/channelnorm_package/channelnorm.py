"""ChannelNorm (per-pixel L2 norm over channels): autograd Function + Module over the
``channelnorm_cuda`` extension.

Same public names and signatures as the reference wrapper
(networks/channelnorm_package/channelnorm.py:5-38): ``ChannelNormFunction.apply(input1, norm_deg)``
and ``ChannelNorm(norm_deg=2)``.  ``norm_deg`` is stored and passed on but, as in the reference
kernels, only the L2 norm is implemented.  The backward honours grad_output's strides (the
reference reads the non-contiguous slice autograd hands it as if it were contiguous).
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import channelnorm_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

_DTYPES = (torch.float32, torch.float16, torch.float64, torch.bfloat16)


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _forward(input1, norm_deg):
    refuse(input1.is_contiguous(), "ChannelNormFunction: input1 must be contiguous (reference channelnorm.py:9)")
    return channelnorm_cuda.forward_alloc(input1, norm_deg)


def _fake_input(input1, op):
    refuse(input1.dim() == 4, op, ": input1 must be 4-D")
    refuse(input1.dtype in _DTYPES, op, ": unsupported dtype ", input1.dtype, " (float, half, double or bfloat16 expected)")


def _forward_fake(input1, norm_deg):
    _fake_input(input1, "fn2::channelnorm")
    return input1.new_empty((input1.shape[0], 1, input1.shape[2], input1.shape[3]))


def _backward_fake(input1, output, grad_output, norm_deg):
    _fake_input(input1, "fn2::channelnorm_backward")
    refuse(grad_output.shape == output.shape, "fn2::channelnorm_backward: gradOutput ", tuple(grad_output.shape), " must match output ",
           tuple(output.shape))
    return input1.new_empty(input1.shape)


def _setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output)
    ctx.norm_deg = inputs[1]


def _grad(ctx, grad_output):
    input1, output = ctx.saved_tensors
    return _backward_op(input1, output, grad_output, ctx.norm_deg), None


_forward_op = fn2_ops.define("channelnorm", "(Tensor input1, int norm_deg) -> Tensor", _forward, _forward_fake, _grad, _setup)
_backward_op = fn2_ops.define("channelnorm_backward", "(Tensor input1, Tensor output, Tensor grad_output, int norm_deg) -> Tensor",
                              channelnorm_cuda.backward_alloc, _backward_fake)


class ChannelNormFunction(Function):
    """``apply`` = the C++ autograd node ``channelnorm_cuda.apply``; ``forward`` / ``backward`` are the same two calls in Python."""

    @classmethod
    def apply(cls, input1, norm_deg=2):
        assert input1.is_contiguous(), "input1 must be contiguous (reference channelnorm.py:9)"
        return channelnorm_cuda.apply(input1, norm_deg)

    @staticmethod
    def forward(ctx, input1, norm_deg=2):
        assert input1.is_contiguous(), "input1 must be contiguous (reference channelnorm.py:9)"
        if torch.compiler.is_compiling():   # Dynamo traces apply() through this method: the operator it can see
            output = _forward_op(input1, norm_deg)
        else:
            output = channelnorm_cuda.forward_alloc(input1, norm_deg)   # (B, 1, H, W), allocated on the C++ side, fully written
        ctx.save_for_backward(input1, output)
        ctx.norm_deg = norm_deg
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, output = ctx.saved_tensors
        backward_alloc = _backward_op if torch.compiler.is_compiling() else channelnorm_cuda.backward_alloc
        return backward_alloc(input1, output, grad_output, ctx.norm_deg), None


class ChannelNorm(nn.Module):
    def __init__(self, norm_deg=2):
        super().__init__()
        self.norm_deg = norm_deg

    def forward(self, input1):
        return ChannelNormFunction.apply(input1, self.norm_deg)
