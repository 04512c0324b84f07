"""Correlation1d: the horizontal-search cost volume of stereo networks (DispNetC and its descendants) -- autograd Function +
Module over the ``correlation1d_cuda`` extension (csrc/binding/correlation1d_cuda.cpp, csrc/correlation_1d.hip).

    out[n, o, y, x] = mean_c in1[n, c, y*s1, x1] * in2[n, c, y*s1, x1 + t*s2],   x1 = x*s1 + md - pad, t = t_min + o

with t over -md//s2 .. md//s2 (``single_direction=0``), -md//s2 .. 0 (``-1``) or 0 .. md//s2 (``+1``); semantics, bounds and the
kernels' domains are documented in include/flownet2_hip_ext.h.  Importing this module fails loudly if the extension has not
been built: the HIP kernels are the only implementation.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import correlation1d_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

_DTYPES = (torch.float32, torch.float16, torch.float64, torch.bfloat16)


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def correlation1d_output_shape(H, W, pad_size, max_displacement, stride1, stride2, single_direction, op="fn2::correlation1d"):
    """(nOut, oH, oW) as fn2x_correlation1d_output_shape gives them (csrc/correlation_1d.hip), in integer arithmetic a symbolic
    size passes through; RuntimeError where the C function returns FN2_EINVAL."""
    refuse(pad_size >= 0 and max_displacement >= 0 and stride1 >= 1 and stride2 >= 1 and -1 <= single_direction <= 1, op,
           ": HIP call failed: invalid argument (pad_size, max_displacement >= 0, stride1, stride2 >= 1 and single_direction in "
           "-1, 0, 1 expected)")
    span = W + 2 * pad_size - 2 * max_displacement
    refuse(H >= 1 and W >= 1 and span >= 1, op, ": HIP call failed: invalid argument (the output would be empty)")
    dr = max_displacement // stride2
    return (2 * dr + 1 if single_direction == 0 else dr + 1), (H + stride1 - 1) // stride1, (span + stride1 - 1) // stride1


def _fake_pair(input1, input2, op):
    """check_pair of binding_common.h, as far as shapes and dtypes decide it."""
    refuse(input1.dtype == input2.dtype, op, ": input2 has dtype ", input2.dtype, ", expected ", input1.dtype)
    refuse(input1.dim() == 4 and input2.dim() == 4, op, ": inputs must be 4-D (N, C, H, W)")
    refuse(input1.shape == input2.shape, op, ": input1 ", tuple(input1.shape), " and input2 ", tuple(input2.shape),
           " must have the same shape")
    refuse(input1.dtype in _DTYPES, op, ": unsupported dtype ", input1.dtype, " (float, half, double or bfloat16 expected)")


def _forward_fake(input1, input2, pad_size, max_displacement, stride1, stride2, single_direction):
    _fake_pair(input1, input2, "fn2::correlation1d")
    n_out, oH, oW = correlation1d_output_shape(input1.shape[2], input1.shape[3], pad_size, max_displacement, stride1, stride2,
                                               single_direction)
    return input1.new_empty((input1.shape[0], n_out, oH, oW))


def _backward_fake(input1, input2, grad_output, pad_size, max_displacement, stride1, stride2, single_direction):
    _fake_pair(input1, input2, "fn2::correlation1d_backward")
    return input1.new_empty(input1.shape), input1.new_empty(input1.shape)


def _setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.corr_params = tuple(inputs[2:])


def _grad(ctx, grad_output):
    input1, input2 = ctx.saved_tensors
    grad_input1, grad_input2 = _backward_op(input1, input2, grad_output, *ctx.corr_params)
    return (grad_input1, grad_input2) + (None,) * 5


_ARGS = "int pad_size, int max_displacement, int stride1, int stride2, int single_direction"
_forward_op = fn2_ops.define("correlation1d", f"(Tensor input1, Tensor input2, {_ARGS}) -> Tensor",
                             correlation1d_cuda.forward_alloc, _forward_fake, _grad, _setup)
_backward_op = fn2_ops.define("correlation1d_backward", f"(Tensor input1, Tensor input2, Tensor grad_output, {_ARGS}) -> (Tensor, Tensor)",
                              correlation1d_cuda.backward_alloc, _backward_fake)


class Correlation1dFunction(Function):
    """``apply`` goes straight to the autograd node the extension implements in C++ (``correlation1d_cuda.apply``); ``forward`` /
    ``backward`` are the same two calls for code that drives a Function's static methods itself -- through the ``fn2`` operators
    while ``torch.compile`` traces, which is how it sees ``apply``."""

    @classmethod
    def apply(cls, input1, input2, pad_size=0, max_displacement=0, stride1=1, stride2=1, single_direction=0):
        return correlation1d_cuda.apply(input1, input2, pad_size, max_displacement, stride1, stride2, single_direction)

    @staticmethod
    def forward(ctx, input1, input2, pad_size=0, max_displacement=0, stride1=1, stride2=1, single_direction=0):
        ctx.save_for_backward(input1, input2)
        ctx.corr_params = (pad_size, max_displacement, stride1, stride2, single_direction)
        if torch.compiler.is_compiling():
            return _forward_op(input1, input2, *ctx.corr_params)
        return correlation1d_cuda.forward_alloc(input1, input2, *ctx.corr_params)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
        if torch.compiler.is_compiling():
            grad_input1, grad_input2 = _backward_op(input1, input2, grad_output, *ctx.corr_params)
        else:
            grad_input1, grad_input2 = correlation1d_cuda.backward_alloc(input1, input2, grad_output, *ctx.corr_params)
        return (grad_input1, grad_input2) + (None,) * 5


class Correlation1d(nn.Module):
    def __init__(self, pad_size=0, max_displacement=0, stride1=1, stride2=1, single_direction=0):
        super().__init__()
        self.pad_size = pad_size
        self.max_displacement = max_displacement
        self.stride1 = stride1
        self.stride2 = stride2
        self.single_direction = single_direction

    def forward(self, input1, input2):
        return Correlation1dFunction.apply(input1, input2, self.pad_size, self.max_displacement, self.stride1, self.stride2,
                                           self.single_direction)

    def extra_repr(self):
        return (f"pad_size={self.pad_size}, max_displacement={self.max_displacement}, stride1={self.stride1}, "
                f"stride2={self.stride2}, single_direction={self.single_direction}")
