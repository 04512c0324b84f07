"""Correlation layer: autograd Function + Module over the ``correlation_cuda`` extension.

Same public names, argument order and defaults as the reference wrapper
(networks/correlation_package/correlation.py:6-60): ``CorrelationFunction.apply(input1, input2,
pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)`` and
``Correlation(pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1)``.
The extension is the gfx950 HIP implementation (csrc/binding/correlation_cuda.cpp); importing this
module fails loudly if it has not been built.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import correlation_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

_DTYPES = (torch.float32, torch.float16, torch.float64, torch.bfloat16)


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _ceil_div(a, b):
    return -((-a) // b)


def _fake_pair(input1, input2, op):
    """check_pair of binding_common.h, as far as shapes and dtypes decide it."""
    refuse(input1.dtype == input2.dtype, op, ": input2 has dtype ", input2.dtype, ", expected ", input1.dtype)
    refuse(input1.dim() == 4 and input2.dim() == 4, op, ": inputs must be 4-D (N, C, H, W)")
    refuse(input1.shape == input2.shape, op, ": input1 ", tuple(input1.shape), " and input2 ", tuple(input2.shape),
           " must have the same shape")
    refuse(input1.dtype in _DTYPES, op, ": unsupported dtype ", input1.dtype, " (float, half, double or bfloat16 expected)")


def correlation_output_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2, op="fn2::correlation"):
    """(nOut, oH, oW) as fn2_correlation_output_shape gives them (csrc/capi.hip), in integer arithmetic a symbolic size passes
    through; RuntimeError where the C function returns FN2_EINVAL."""
    refuse(pad_size >= 0 and kernel_size >= 1 and max_displacement >= 0 and stride1 >= 1 and stride2 >= 1, op,
           ": HIP call failed: invalid argument (pad_size, max_displacement >= 0 and kernel_size, stride1, stride2 >= 1 expected)")
    border = (kernel_size - 1) // 2 + max_displacement
    d = (max_displacement // stride2) * 2 + 1
    oH, oW = _ceil_div(H + 2 * pad_size - 2 * border, stride1), _ceil_div(W + 2 * pad_size - 2 * border, stride1)
    refuse(H >= 1 and W >= 1 and oH >= 1 and oW >= 1, op, ": HIP call failed: invalid argument (the output would be empty)")
    return d * d, oH, oW


def _correlation_fake(input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply):
    _fake_pair(input1, input2, "fn2::correlation")
    n_out, oH, oW = correlation_output_shape(input1.shape[2], input1.shape[3], pad_size, kernel_size, max_displacement, stride1, stride2)
    return input1.new_empty((input1.shape[0], n_out, oH, oW))


def _correlation_backward_fake(input1, input2, grad_output, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply):
    _fake_pair(input1, input2, "fn2::correlation_backward")
    return input1.new_empty(input1.shape), input1.new_empty(input1.shape)


def _correlation_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.corr_params = tuple(inputs[2:])


def _correlation_grad(ctx, grad_output):
    input1, input2 = ctx.saved_tensors
    grad_input1, grad_input2 = _correlation_backward_op(input1, input2, grad_output, *ctx.corr_params)
    return (grad_input1, grad_input2) + (None,) * 6


_CORR_ARGS = "int pad_size, int kernel_size, int max_displacement, int stride1, int stride2"
_correlation_op = fn2_ops.define(
    "correlation", f"(Tensor input1, Tensor input2, {_CORR_ARGS}, int corr_multiply) -> Tensor",
    correlation_cuda.forward_alloc, _correlation_fake, _correlation_grad, _correlation_setup)
_correlation_backward_op = fn2_ops.define(
    "correlation_backward", f"(Tensor input1, Tensor input2, Tensor grad_output, {_CORR_ARGS}, int corr_multiply) -> (Tensor, Tensor)",
    correlation_cuda.backward_alloc, _correlation_backward_fake)


def _leakyrelu_cat(input1, input2, redir, pad_size, kernel_size, max_displacement, stride1, stride2, negative_slope):
    """The concat buffer allocated, its first channels copied and the fused kernel: CorrelationLeakyReLUCatFunction.forward."""
    n_out = ((max_displacement // stride2) * 2 + 1) ** 2
    B, Cr, oH, oW = redir.shape
    buf = redir.new_empty((B, Cr + n_out, oH, oW))
    buf[:, :Cr].copy_(redir)
    with torch.cuda.device_of(input1):
        correlation_cuda.forward_fused(input1, input2, buf, Cr, negative_slope, pad_size, kernel_size, max_displacement, stride1, stride2)
    return buf


def _leakyrelu_cat_fake(input1, input2, redir, pad_size, kernel_size, max_displacement, stride1, stride2, negative_slope):
    op = "fn2::correlation_leakyrelu_cat"
    _fake_pair(input1, input2, op)
    refuse(redir.dtype == input1.dtype, op, ": redir has dtype ", redir.dtype, ", expected ", input1.dtype)
    refuse(redir.dim() == 4, op, ": redir must be 4-D")
    n_out, oH, oW = correlation_output_shape(input1.shape[2], input1.shape[3], pad_size, kernel_size, max_displacement, stride1, stride2, op)
    refuse(redir.shape[0] == input1.shape[0] and redir.shape[2] == oH and redir.shape[3] == oW, op, ": a buffer over redir ",
           tuple(redir.shape), " cannot hold ", n_out, " channels of ", oH, "x", oW)
    return redir.new_empty((redir.shape[0], redir.shape[1] + n_out, oH, oW))


def _leakyrelu_cat_backward(input1, input2, buf, grad_buf, channel_offset, negative_slope, pad_size, kernel_size, max_displacement,
                            stride1, stride2):
    with torch.cuda.device_of(input1):
        grad_in1, grad_in2 = input1.new_empty(0), input2.new_empty(0)
        correlation_cuda.backward_fused(input1, input2, buf, grad_buf, channel_offset, negative_slope, grad_in1, grad_in2, pad_size,
                                        kernel_size, max_displacement, stride1, stride2)
    return grad_in1, grad_in2


def _leakyrelu_cat_backward_fake(input1, input2, buf, grad_buf, channel_offset, negative_slope, pad_size, kernel_size, max_displacement,
                                 stride1, stride2):
    _fake_pair(input1, input2, "fn2::correlation_leakyrelu_cat_backward")
    refuse(grad_buf.shape == buf.shape, "fn2::correlation_leakyrelu_cat_backward: gradBuffer ", tuple(grad_buf.shape),
           " must have the buffer's shape ", tuple(buf.shape))
    return input1.new_empty(input1.shape), input1.new_empty(input1.shape)


def _slope_differentiates(negative_slope, want1, want2):
    if not negative_slope > 0 and (want1 or want2):
        raise ValueError("CorrelationLeakyReLUCatFunction differentiates only for negative_slope > 0")


def _leakyrelu_cat_setup(ctx, inputs, output):
    input1, input2, redir = inputs[:3]
    _slope_differentiates(inputs[8], ctx.needs_input_grad[0], ctx.needs_input_grad[1])
    ctx.save_for_backward(input1, input2, output)
    ctx.corr_params = tuple(inputs[3:8])
    ctx.channel_offset, ctx.negative_slope = redir.shape[1], inputs[8]


def _leakyrelu_cat_grad(ctx, grad_buf):
    input1, input2, buf = ctx.saved_tensors
    Cr = ctx.channel_offset
    grad_in1 = grad_in2 = None
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
        grad_in1, grad_in2 = _leakyrelu_cat_backward_op(input1, input2, buf, grad_buf, Cr, ctx.negative_slope, *ctx.corr_params)
    grad_redir = grad_buf[:, :Cr] if ctx.needs_input_grad[2] else None
    return (grad_in1, grad_in2, grad_redir) + (None,) * 6


_leakyrelu_cat_op = fn2_ops.define(
    "correlation_leakyrelu_cat", f"(Tensor input1, Tensor input2, Tensor redir, {_CORR_ARGS}, float negative_slope) -> Tensor",
    _leakyrelu_cat, _leakyrelu_cat_fake, _leakyrelu_cat_grad, _leakyrelu_cat_setup)
_leakyrelu_cat_backward_op = fn2_ops.define(
    "correlation_leakyrelu_cat_backward",
    f"(Tensor input1, Tensor input2, Tensor buffer, Tensor grad_buffer, int channel_offset, float negative_slope, {_CORR_ARGS})"
    " -> (Tensor, Tensor)", _leakyrelu_cat_backward, _leakyrelu_cat_backward_fake)


class CorrelationFunction(Function):
    """out[n, tj*D+ti, y, x] = mean_c in1[n,c,y',x'] * in2[n,c,y'+tj*s2,x'+ti*s2] (reference
    correlation_cuda_kernel.cu:73-147); backward per :150-334.

    ``apply`` goes straight to the autograd node the extension implements in C++ (``correlation_cuda.apply``: no Python between
    ``apply`` and the launch, no GIL in the backward); ``forward`` / ``backward`` below are the same two calls for code written
    against the reference's static methods."""

    @classmethod
    def apply(cls, input1, input2, pad_size=3, kernel_size=3, max_displacement=20, stride1=1, stride2=2, corr_multiply=1):
        return correlation_cuda.apply(input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)

    @staticmethod
    def forward(ctx, input1, input2, pad_size=3, kernel_size=3, max_displacement=20, stride1=1, stride2=2,
                corr_multiply=1):
        ctx.save_for_backward(input1, input2)
        ctx.corr_params = (pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)
        if torch.compiler.is_compiling():   # Dynamo traces apply() through this method: the operator it can see
            return _correlation_op(input1, input2, *ctx.corr_params)
        # correlation_cuda.forward with the reference's three empty tensors (correlation.py:20-22) created and sized on the C++
        # side: one call, device guard included
        return correlation_cuda.forward_alloc(input1, input2, *ctx.corr_params)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
        if torch.compiler.is_compiling():
            grad_input1, grad_input2 = _correlation_backward_op(input1, input2, grad_output, *ctx.corr_params)
        else:
            grad_input1, grad_input2 = correlation_cuda.backward_alloc(input1, input2, grad_output, *ctx.corr_params)
        return (grad_input1, grad_input2) + (None,) * 6


class Correlation(nn.Module):
    def __init__(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1):
        super().__init__()
        self.pad_size = pad_size
        self.kernel_size = kernel_size
        self.max_displacement = max_displacement
        self.stride1 = stride1
        self.stride2 = stride2
        self.corr_multiply = corr_multiply

    def forward(self, input1, input2):
        return CorrelationFunction.apply(input1, input2, self.pad_size, self.kernel_size, self.max_displacement,
                                         self.stride1, self.stride2, self.corr_multiply)

    def extra_repr(self):
        return (f"pad_size={self.pad_size}, kernel_size={self.kernel_size}, max_displacement={self.max_displacement}, "
                f"stride1={self.stride1}, stride2={self.stride2}")


class CorrelationLeakyReLUCatFunction(Function):
    """``cat((redir, leaky_relu(corr(input1, input2), slope)), 1)`` (FlowNetC.py:86-87, :92) as one differentiable op: forward =
    the correlation kernel with the activation and the store into the concat buffer fused into its epilogue; backward = the
    gradient of the buffer's correlation slice read in place, the activation's derivative taken from the sign of the stored
    output (no mask, no saved pre-activation), the correlation backward kernels (correlation_cuda.backward_fused).
    ``apply`` = the C++ autograd node ``correlation_cuda.leakyrelu_cat_apply``; the static methods are the same calls in Python."""

    @classmethod
    def apply(cls, input1, input2, redir, pad_size, kernel_size, max_displacement, stride1, stride2, negative_slope):
        if not negative_slope > 0 and (input1.requires_grad or input2.requires_grad):
            raise ValueError("CorrelationLeakyReLUCatFunction differentiates only for negative_slope > 0")
        return correlation_cuda.leakyrelu_cat_apply(input1, input2, redir, pad_size, kernel_size, max_displacement, stride1, stride2,
                                                    float(negative_slope))

    @staticmethod
    def forward(ctx, input1, input2, redir, pad_size, kernel_size, max_displacement, stride1, stride2, negative_slope):
        if torch.compiler.is_compiling():   # (inside the traced node the inputs are detached: autograd is asked instead)
            _slope_differentiates(negative_slope, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
            Cr = redir.shape[1]
            buf = _leakyrelu_cat_op(input1, input2, redir, pad_size, kernel_size, max_displacement, stride1, stride2, float(negative_slope))
        else:
            _slope_differentiates(negative_slope, input1.requires_grad, input2.requires_grad)
            Cr = redir.shape[1]
            buf = _leakyrelu_cat(input1, input2, redir, pad_size, kernel_size, max_displacement, stride1, stride2, float(negative_slope))
        ctx.save_for_backward(input1, input2, buf)
        ctx.corr_params = (pad_size, kernel_size, max_displacement, stride1, stride2)
        ctx.channel_offset, ctx.negative_slope = Cr, float(negative_slope)
        return buf

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_buf):
        input1, input2, buf = ctx.saved_tensors
        Cr = ctx.channel_offset
        grad_in1 = grad_in2 = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            fused_backward = _leakyrelu_cat_backward_op if torch.compiler.is_compiling() else _leakyrelu_cat_backward
            grad_in1, grad_in2 = fused_backward(input1, input2, buf, grad_buf, Cr, ctx.negative_slope, *ctx.corr_params)
        grad_redir = grad_buf[:, :Cr] if ctx.needs_input_grad[2] else None
        return (grad_in1, grad_in2, grad_redir) + (None,) * 6


class CorrelationLeakyReLUCat(nn.Module):
    """``torch.cat((redir, leaky_relu(corr(input1, input2), slope)), 1)`` with the activation and the concat
    fused into the correlation epilogue -- the three statements FlowNetC.py:86-87,92 as one kernel pass over the 441-channel
    cost volume instead of three --, and, in training, one pass instead of two in front of the correlation backward
    (``CorrelationLeakyReLUCatFunction``).

        cat = CorrelationLeakyReLUCat(20, 1, 20, 1, 2, negative_slope=0.1)(out_conv3a, out_conv3b, out_conv_redir)
    """

    def __init__(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, negative_slope=0.1):
        super().__init__()
        # the backward reads the activation's derivative off the sign of the stored output: only an increasing activation
        # (slope > 0) keeps that sign (fn2_correlation_backward_fused rejects anything else) -- say so here, not in backward()
        if not negative_slope > 0:
            raise ValueError(f"CorrelationLeakyReLUCat needs negative_slope > 0 (got {negative_slope}); for ReLU or a negative "
                             "slope compose Correlation, the activation and torch.cat")
        self.corr_params = (pad_size, kernel_size, max_displacement, stride1, stride2)
        self.negative_slope = negative_slope

    def forward(self, input1, input2, redir):
        return CorrelationLeakyReLUCatFunction.apply(input1, input2, redir, *self.corr_params, self.negative_slope)
