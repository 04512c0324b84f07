"""Correlation1d: the horizontal-search cost volume of stereo networks (DispNetC and its descendants) -- autograd Function +
Module over the ``correlation1d_cuda`` extension (csrc/binding/correlation1d_cuda.cpp, csrc/correlation_1d.hip).

    out[n, o, y, x] = mean_c in1[n, c, y*s1, x1] * in2[n, c, y*s1, x1 + t*s2],   x1 = x*s1 + md - pad, t = t_min + o

with t over -md//s2 .. md//s2 (``single_direction=0``), -md//s2 .. 0 (``-1``) or 0 .. md//s2 (``+1``); semantics, bounds and the
kernels' domains are documented in include/flownet2_hip_ext.h.  Importing this module fails loudly if the extension has not
been built: the HIP kernels are the only implementation.
"""
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import correlation1d_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose


class Correlation1dFunction(Function):
    """``apply`` goes straight to the autograd node the extension implements in C++ (``correlation1d_cuda.apply``); ``forward`` /
    ``backward`` are the same two calls for code that drives a Function's static methods itself."""

    @classmethod
    def apply(cls, input1, input2, pad_size=0, max_displacement=0, stride1=1, stride2=1, single_direction=0):
        return correlation1d_cuda.apply(input1, input2, pad_size, max_displacement, stride1, stride2, single_direction)

    @staticmethod
    def forward(ctx, input1, input2, pad_size=0, max_displacement=0, stride1=1, stride2=1, single_direction=0):
        ctx.save_for_backward(input1, input2)
        ctx.corr_params = (pad_size, max_displacement, stride1, stride2, single_direction)
        return correlation1d_cuda.forward_alloc(input1, input2, *ctx.corr_params)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
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
