"""CorrPyramid (incubating): the BUILD of RAFT's all-pairs correlation pyramid -- what ``CorrBlock.__init__`` (``core/corr.py``) composes
from ``torch.matmul``, a division by sqrt(C) and one ``avg_pool2d`` per further level -- as one fused MFMA kernel; autograd Function +
Module over the ``corr_pyramid_cuda`` extension (csrc/binding/corr_pyramid_cuda.cpp, csrc/corr_pyramid.hip).

    level 0      [p, 0, v, u] = fl32(s * sum_c fmap1[b, c, y, x] fmap2[b, c, v, u]),  p = (b H + y) W + x,  s = fl32(1 / sqrt(C))
    level l + 1  [p, 0, v, u] = fl32(((a + b) + (c + d)) * 0.25) over the 2 x 2 block of level l, sizes H2 >> l x W2 >> l

The sum runs on the bf16 matrix cores through the exact three-term split (csrc/bf16x3.h); every element of every level is written
once, by the kernel that computed it, and never read back.  The backward folds the levels' gradients into the gradient of the
volume in one streaming kernel and contracts it with the two maps (``at::bmm``).  float32, contiguous maps only.  Semantics, bounds
and the checks are documented in include/preview/flownet2_hip_pyramid.h.  Importing this module fails loudly if the extension has
not been built: the HIP kernels are the only implementation.
"""
import sys
import types

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import corr_pyramid_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

KERNEL_LEVELS = 4   # FN2Y_MAX_LEVELS (include/preview/flownet2_hip_pyramid.h): what one launch builds
MAX_LEVELS = 8      # FN2P_MAX_LEVELS: what the lookup takes; levels beyond KERNEL_LEVELS are pooled from the last one here

# STATUS_PYRAMID of csrc/binding/binding_status.h, for the fake implementations (tests/test_corr_pyramid_host.py compares the two)
_EINVAL = "invalid shape, layout or parameter (contiguous maps, 1 .. 4 levels, none of them empty)"
_EDTYPE = "dtype not supported by this op (float32 only: convert with .float())"


def _status(op, text, code):
    return f"{op}: HIP call failed: flownet2_hip_pyramid: {text} (code {code})"


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _fake_inputs(fmap1, fmap2, num_levels, op):
    """check_inputs of csrc/binding/corr_pyramid_cuda.cpp and check 1 of the C ABI, as far as shapes and dtypes decide them."""
    refuse(fmap2.dtype == fmap1.dtype, op, ": fmap2 has dtype ", fmap2.dtype, ", expected ", fmap1.dtype)
    refuse(fmap1.dtype == torch.float32, _status(op, _EDTYPE, -2))
    refuse(fmap1.dim() == 4 and fmap2.dim() == 4 and fmap1.shape[0] == fmap2.shape[0] and fmap1.shape[1] == fmap2.shape[1], op, ": fmap1 ",
           tuple(fmap1.shape), " and fmap2 ", tuple(fmap2.shape), " must be [B, C, H, W] and [B, C, H2, W2]")
    refuse(fmap1.is_contiguous() and fmap2.is_contiguous() and 1 <= num_levels <= KERNEL_LEVELS, _status(op, _EINVAL, -1))
    top = 2 ** (num_levels - 1)
    refuse(fmap1.shape[1] >= 1 and fmap1.shape[2] >= 1 and fmap1.shape[3] >= 1 and fmap2.shape[2] // top >= 1 and fmap2.shape[3] // top >= 1,
           _status(op, _EINVAL, -1))


def _forward_fake(fmap1, fmap2, num_levels):
    _fake_inputs(fmap1, fmap2, num_levels, "corr_pyramid_cuda.forward")
    pixels = fmap1.shape[0] * fmap1.shape[2] * fmap1.shape[3]
    return [fmap1.new_empty((pixels, 1, fmap2.shape[2] // 2 ** l, fmap2.shape[3] // 2 ** l)) for l in range(num_levels)]


def _backward_fake(fmap1, fmap2, grad_levels):
    op = "corr_pyramid_cuda.backward"
    _fake_inputs(fmap1, fmap2, len(grad_levels), op)
    pixels = fmap1.shape[0] * fmap1.shape[2] * fmap1.shape[3]
    for l, g in enumerate(grad_levels):
        if g is None:
            continue
        refuse(g.dtype == fmap1.dtype, op, ": a level's gradient has dtype ", g.dtype, ", expected ", fmap1.dtype)
        four = g.dim() == 4 and g.shape[1] == 1
        refuse((four or g.dim() == 3) and g.shape[0] == pixels and g.shape[-2] == fmap2.shape[2] // 2 ** l
               and g.shape[-1] == fmap2.shape[3] // 2 ** l, op, ": the gradient of level ", l, " has shape ", tuple(g.shape))
    return fmap1.new_empty(fmap1.shape), fmap2.new_empty(fmap2.shape)


def _backward_impl(fmap1, fmap2, grad_levels):
    return corr_pyramid_cuda.backward_alloc(fmap1, fmap2, list(grad_levels))


def _setup(ctx, inputs, output):
    fmap1, fmap2, _ = inputs
    ctx.save_for_backward(fmap1, fmap2)


def _grad(ctx, grads):
    fmap1, fmap2 = ctx.saved_tensors
    g1, g2 = _backward_op(fmap1, fmap2, list(grads))
    return g1, g2, None


_forward_op = fn2_ops.define("corr_pyramid", "(Tensor fmap1, Tensor fmap2, int num_levels) -> Tensor[]",
                             corr_pyramid_cuda.forward_alloc, _forward_fake, _grad, _setup, incubating=True)
_backward_op = fn2_ops.define("corr_pyramid_backward", "(Tensor fmap1, Tensor fmap2, Tensor?[] grad_levels) -> (Tensor, Tensor)",
                              _backward_impl, _backward_fake, incubating=True)


class CorrPyramidFunction(Function):
    """``apply(fmap1, fmap2, num_levels)`` (num_levels <= 4) goes straight to the autograd node the extension implements in C++
    (``corr_pyramid_cuda.apply``) and returns the levels; ``forward`` / ``backward`` are the same two calls for code that drives a
    Function's static methods itself -- through the ``fn2`` operators while ``torch.compile`` traces, which is how it sees ``apply``."""

    @classmethod
    def apply(cls, fmap1, fmap2, num_levels):
        return tuple(corr_pyramid_cuda.apply(fmap1, fmap2, num_levels))

    @staticmethod
    def forward(ctx, fmap1, fmap2, num_levels):
        ctx.save_for_backward(fmap1, fmap2)
        if torch.compiler.is_compiling():
            return tuple(_forward_op(fmap1, fmap2, num_levels))
        return tuple(corr_pyramid_cuda.forward_alloc(fmap1, fmap2, num_levels))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        fmap1, fmap2 = ctx.saved_tensors
        if torch.compiler.is_compiling():
            g1, g2 = _backward_op(fmap1, fmap2, list(grads))
        else:
            g1, g2 = corr_pyramid_cuda.backward_alloc(fmap1, fmap2, list(grads), ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return g1, g2, None


def corr_pyramid(fmap1, fmap2, num_levels):
    """The all-pairs correlation pyramid of ``fmap1`` (B x C x H x W) and ``fmap2`` (B x C x H2 x W2), float32 and contiguous: a list
    of ``num_levels`` tensors (B H W) x 1 x (H2 >> l) x (W2 >> l), equal in meaning to ``CorrBlock.__init__``'s composition and
    differentiable in both maps.  One kernel builds up to four levels; further ones are pooled from the fourth with ``avg_pool2d``."""
    levels = list(CorrPyramidFunction.apply(fmap1, fmap2, min(num_levels, KERNEL_LEVELS)))
    for _ in range(num_levels - KERNEL_LEVELS):
        levels.append(F.avg_pool2d(levels[-1], 2, stride=2))
    return levels


class _CallableModule(types.ModuleType):
    """This module and its main function share a name, so once the module is imported ``from networks.correlation_package import
    corr_pyramid`` finds the module, not the function the package's ``_HOME`` promises: calling the module calls the function."""

    def __call__(self, fmap1, fmap2, num_levels):
        return corr_pyramid(fmap1, fmap2, num_levels)


sys.modules[__name__].__class__ = _CallableModule


class CorrPyramid(nn.Module):
    """``CorrPyramid(num_levels)(fmap1, fmap2)`` -> the list of levels."""

    def __init__(self, num_levels=4):
        super().__init__()
        self.num_levels = num_levels

    def forward(self, fmap1, fmap2):
        return corr_pyramid(fmap1, fmap2, self.num_levels)

    def extra_repr(self):
        return f"num_levels={self.num_levels}"
