"""The structural-similarity distance, the SSIM photometric term of unsupervised optical flow (ARFlow, UFlow) and of unsupervised
stereo and depth (monodepth: 0.85 SSIM + 0.15 L1), as an autograd Function + Modules over the ``ssim_cuda`` extension
(csrc/binding/ssim_cuda.cpp, csrc/ssim.hip).  A staging layer (build.STAGING): its interface may still change.

    over the k x k window at p, k = 2 md + 1:    mx, my the means, sx, sy the variances, sxy the covariance
    S = (2 mx my + c1)(2 sxy + c2) / ((mx^2 + my^2 + c1)(sx + sy + c2))        dist[n, c, p] = clamp((1 - S) / 2, 0, 1)

``im1`` and ``im2`` are float32 N x C x H x W, any C; the result has their shape.  ``border="zero"`` is ARFlow's ``SSIM`` with its
valid-only result embedded: exactly 0 on the border ring of width md, which sends no gradient; ``border="reflect"`` is monodepth2's
``SSIM`` module: both images reflection-padded by md, every pixel has a value.  Both images get gradients; the backward is a gather
without atomics and bit-reproducible.  One kernel each way replaces the composition's five ``avg_pool2d`` calls, its elementwise
launches and their N x C x H x W temporaries.  Semantics, arithmetic order and bounds are documented in
include/staging/flownet2_hip_ssim.h.  Importing this module fails loudly if the extension has not been built: the HIP kernels are
the only implementation.
"""
import ctypes

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import ssim_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

BORDERS = {"zero": ssim_cuda.BORDER_ZERO, "reflect": ssim_cuda.BORDER_REFLECT}


def _border_code(border):
    if border not in BORDERS:
        raise ValueError(f"ssim: border {border!r} is not 'zero' or 'reflect'")
    return BORDERS[border]


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _f32(v):
    """``(float)v`` of the binding: the float32 nearest to a Python float (0 for one that underflows, inf for one that overflows)."""
    return ctypes.c_float(v).value


def _fake_inputs(im1, im2, max_distance, c1, c2, border, op):
    """check_inputs of csrc/binding/ssim_cuda.cpp, as far as shapes, dtypes and parameters decide it."""
    refuse(im1.dim() == 4 and im2.dim() == 4, op, ": im1 and im2 must be 4-D (N, C, H, W); add the missing dimensions with [None]")
    refuse(im1.shape == im2.shape, op, ": im2 ", tuple(im2.shape), " must have the shape of im1 ", tuple(im1.shape))
    refuse(im1.shape[1] >= 1 and im1.shape[2] >= 1 and im1.shape[3] >= 1, op, ": the images ", tuple(im1.shape),
           " have an empty channel, row or column dimension")
    refuse(1 <= max_distance <= ssim_cuda.MAX_DISTANCE, op, ": max_distance ", max_distance, " is not 1, 2 or 3")
    refuse(0.0 < _f32(c1) < float("inf"), op, ": c1 ", c1, " is not a finite float above 0")   # as the binding: after the cast to float
    refuse(0.0 < _f32(c2) < float("inf"), op, ": c2 ", c2, " is not a finite float above 0")
    refuse(border in (ssim_cuda.BORDER_ZERO, ssim_cuda.BORDER_REFLECT), op, ": border code ", border, " is not 0 (zero) or 1 (reflect)")
    refuse(border != ssim_cuda.BORDER_REFLECT or (im1.shape[2] > max_distance and im1.shape[3] > max_distance), op,
           ": border reflect needs H and W above max_distance ", max_distance, ", got ", im1.shape[2], " x ", im1.shape[3],
           ": use border zero or a smaller max_distance")
    for name, t in (("im1", im1), ("im2", im2)):
        refuse(t.dtype == torch.float32, op, ": ", name, " must be float32, got ", t.dtype, ": convert it with .float()")


def _forward_fake(im1, im2, max_distance, c1, c2, border):
    _fake_inputs(im1, im2, max_distance, c1, c2, border, "fn2::ssim")
    return im1.new_empty(im1.shape)


def _backward(im1, im2, grad_output, max_distance, c1, c2, border, want1, want2):
    grad1, grad2 = ssim_cuda.backward_alloc(im1, im2, grad_output, max_distance, c1, c2, border, want1, want2)
    return (grad1 if want1 else im1.new_empty(0)), (grad2 if want2 else im1.new_empty(0))


def _backward_fake(im1, im2, grad_output, max_distance, c1, c2, border, want1, want2):
    _fake_inputs(im1, im2, max_distance, c1, c2, border, "fn2::ssim_backward")
    refuse(want1 or want2, "fn2::ssim_backward: neither gradient is wanted")
    return (im1.new_empty(im1.shape) if want1 else im1.new_empty(0)), (im1.new_empty(im1.shape) if want2 else im1.new_empty(0))


def _setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.options = tuple(inputs[2:])


def _grad(ctx, grad_output):
    im1, im2 = ctx.saved_tensors
    want1, want2 = ctx.needs_input_grad[:2]
    if not (want1 or want2):
        return None, None, None, None, None, None
    grad1, grad2 = _backward_op(im1, im2, grad_output, *ctx.options, want1, want2)
    return (grad1 if want1 else None), (grad2 if want2 else None), None, None, None, None


_forward_op = fn2_ops.define("ssim", "(Tensor im1, Tensor im2, int max_distance, float c1, float c2, int border) -> Tensor",
                             ssim_cuda.forward_alloc, _forward_fake, _grad, _setup, staging=True)
# a gradient that is not wanted comes back with numel 0 (a schema has no optional result) and is not computed
_backward_op = fn2_ops.define(
    "ssim_backward",
    "(Tensor im1, Tensor im2, Tensor grad_output, int max_distance, float c1, float c2, int border, bool want1, bool want2) -> (Tensor, Tensor)",
    _backward, _backward_fake, staging=True)


class SSIMFunction(Function):
    """``apply`` goes straight to the autograd node the extension implements in C++ (``ssim_cuda.apply``);
    ``forward`` / ``backward`` are the same two calls for code that drives a Function's static methods itself.  ``border`` is the
    code (``BORDERS``), not the name."""

    @classmethod
    def apply(cls, im1, im2, max_distance=1, c1=1e-4, c2=9e-4, border=0):
        return ssim_cuda.apply(im1, im2, int(max_distance), float(c1), float(c2), int(border))

    @staticmethod
    def forward(ctx, im1, im2, max_distance=1, c1=1e-4, c2=9e-4, border=0):
        ctx.save_for_backward(im1, im2)
        ctx.options = (int(max_distance), float(c1), float(c2), int(border))
        if torch.compiler.is_compiling():   # Dynamo traces apply() through this method: the operator it can see
            return _forward_op(im1, im2, *ctx.options)
        return ssim_cuda.forward_alloc(im1, im2, *ctx.options)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        im1, im2 = ctx.saved_tensors
        want1, want2 = ctx.needs_input_grad[:2]
        if not (want1 or want2):
            return None, None, None, None, None, None
        if torch.compiler.is_compiling():
            grad1, grad2 = _backward_op(im1, im2, grad_output, *ctx.options, want1, want2)
            return (grad1 if want1 else None), (grad2 if want2 else None), None, None, None, None
        return tuple(ssim_cuda.backward_alloc(im1, im2, grad_output, *ctx.options, want1, want2)) + (None, None, None, None)


def ssim_distance(im1, im2, md=1, c1=1e-4, c2=9e-4, border="zero"):
    """N x C x H x W: ``clamp((1 - SSIM) / 2, 0, 1)`` of the two images over (2 md + 1)^2 windows; ``border`` picks ARFlow's
    valid-only form embedded in zeros ("zero") or monodepth2's reflection padding ("reflect")."""
    return SSIMFunction.apply(im1, im2, md, c1, c2, _border_code(border))


class SSIM(nn.Module):
    """``SSIM(md=1)(im1, im2)`` -> N x C x H x W, ``ssim_distance`` with the parameters kept in the module."""

    def __init__(self, md=1, c1=1e-4, c2=9e-4, border="zero"):
        super().__init__()
        if md not in (1, 2, 3):
            raise ValueError(f"SSIM: md {md!r} is not 1, 2 or 3")
        self.md, self.c1, self.c2, self.border = int(md), float(c1), float(c2), border
        self._code = _border_code(border)

    def forward(self, im1, im2):
        return SSIMFunction.apply(im1, im2, self.md, self.c1, self.c2, self._code)

    def extra_repr(self):
        return f"md={self.md}, c1={self.c1}, c2={self.c2}, border={self.border!r}"


class SSIMLoss(nn.Module):
    """The SSIM photometric loss of ARFlow / monodepth: ``loss(im1, im2_warped, mask=None)`` ->

        sum(dist * valid) / (C * sum(valid) + 1e-6),        valid = the inner rectangle (all ones under "reflect") * mask

    ``mask`` is N x 1 x H x W (an occlusion mask, 1 = use the pixel) or None.  The distance is the HIP kernel; the reduction acts
    on the result and stays in PyTorch."""

    def __init__(self, md=1, border="zero", c1=1e-4, c2=9e-4):
        super().__init__()
        self.ssim = SSIM(md, c1, c2, border)

    def forward(self, im1, im2_warped, mask=None):
        dist = self.ssim(im1, im2_warped)
        N, C, H, W = dist.shape
        md = 0 if self.ssim.border == "reflect" else self.ssim.md
        valid = dist.new_zeros((N, 1, H, W))
        valid[:, :, md:H - md, md:W - md] = 1.0
        if mask is not None:
            if mask.shape != valid.shape:
                raise ValueError(f"SSIMLoss: mask of shape {tuple(mask.shape)} must be N x 1 x H x W = {tuple(valid.shape)}")
            valid = valid * mask
        return (dist * valid).sum() / (C * valid.sum() + 1e-6)
