"""CorrSample and CorrBlock (preview): the lookup of a PREBUILT all-pairs correlation pyramid -- RAFT's default ``CorrBlock``
(``core/corr.py``; ``raft.py`` with ``alternate_corr=False``) and that of its descendants (GMA, RAFT-Stereo, CRAFT, SEA-RAFT) --
autograd Function + Module over the ``corr_sample_cuda`` extension (csrc/binding/corr_sample_cuda.cpp, csrc/corr_sample.hip).

    out[n, l*D*D + i*D + j, y, x] = sum_corners w * level_l[(n*H + y)*W + x, 0, y0 + j - r + oy, x0 + i - r + ox]

with (x0, y0) = floor(coords[n, :, y, x] / 2**l), D = 2 r + 1 and the bilinear weights w of the fractional parts: one kernel in
place of RAFT's ``grid_sample`` per level, concat and permute, and a backward that writes the levels' gradients without atomics,
bit-reproducibly.  The all-pairs matmul and the ``avg_pool2d`` pyramid stay in PyTorch (rocBLAS / MIOpen): they run once per step.
``coords`` (channel 0 = x, 1 = y, in level-0 cells) gets no gradient and must not require one.  float32 only.  Semantics, bounds and
the checks are documented in include/preview/flownet2_hip_sample.h.  Use ``CorrBlock`` when the volume fits in memory,
``AlternateCorrBlock`` (corr_lookup.py) when it does not.  Importing this module fails loudly if the extension has not been built:
the HIP kernels are the only implementation.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import corr_sample_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

MAX_RADIUS = 8   # FN2P_MAX_RADIUS (include/preview/flownet2_hip_sample.h)
MAX_LEVELS = 8   # FN2P_MAX_LEVELS


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _fake_inputs(pyramid, coords, radius, op):
    """check_inputs of csrc/binding/corr_sample_cuda.cpp, as far as shapes and dtypes decide it."""
    refuse(coords.dtype == torch.float32, op, ": coords must be float32, got ", coords.dtype, ": convert it with .float()")
    refuse(1 <= len(pyramid) <= MAX_LEVELS, op, ": the pyramid has ", len(pyramid), " levels, expected 1 .. ", MAX_LEVELS)
    refuse(0 <= radius <= MAX_RADIUS, op, ": radius ", radius, " outside 0 .. ", MAX_RADIUS)
    refuse(coords.dim() == 4 and coords.shape[1] == 2, op, ": coords has shape ", tuple(coords.shape), ", expected [B, 2, H, W]")
    pixels = coords.shape[0] * coords.shape[2] * coords.shape[3]
    for lvl in pyramid:
        refuse(lvl.dtype == torch.float32, op, ": float32 tensors expected, got ", lvl.dtype,
               " (RAFT builds its correlation volume in float: use .float())")
        refuse(((lvl.dim() == 4 and lvl.shape[1] == 1) or lvl.dim() == 3) and lvl.shape[0] == pixels, op, ": a pyramid level has shape ",
               tuple(lvl.shape), ", expected [", pixels, ", 1, H2, W2] for coords ", tuple(coords.shape))


def _forward_fake(pyramid, coords, radius):
    _fake_inputs(pyramid, coords, radius, "fn2::corr_sample")
    return coords.new_empty((coords.shape[0], len(pyramid) * (2 * radius + 1) ** 2, coords.shape[2], coords.shape[3]))


def _backward_fake(pyramid, coords, grad_output, radius):
    _fake_inputs(pyramid, coords, radius, "fn2::corr_sample_backward")
    return [lvl.new_empty(lvl.shape) for lvl in pyramid]


def _no_coords_gradient(wanted):
    # a silent None for coords would train wrongly: RAFT detaches coords in every iteration, and so must the caller
    if wanted:
        raise RuntimeError("CorrSample: coords requires grad, but this layer has no gradient for coords (as RAFT's alt_cuda_corr): "
                           "pass coords.detach()")


def _setup(ctx, inputs, output):
    pyramid, coords, radius = inputs
    _no_coords_gradient(ctx.needs_input_grad[-2])   # (from the end: the flags of a Tensor[] argument may come flattened)
    ctx.save_for_backward(coords, *pyramid)
    ctx.radius = radius


def _grad(ctx, grad_output):
    coords, *pyramid = ctx.saved_tensors
    return _backward_op(pyramid, coords, grad_output, ctx.radius), None, None


_forward_op = fn2_ops.define("corr_sample", "(Tensor[] pyramid, Tensor coords, int radius) -> Tensor",
                             corr_sample_cuda.forward_alloc, _forward_fake, _grad, _setup, preview=True)
_backward_op = fn2_ops.define("corr_sample_backward", "(Tensor[] pyramid, Tensor coords, Tensor grad_output, int radius) -> Tensor[]",
                              corr_sample_cuda.backward_alloc, _backward_fake, preview=True)


class CorrSampleFunction(Function):
    """``apply(coords, radius, *pyramid)`` goes straight to the autograd node the extension implements in C++
    (``corr_sample_cuda.apply``); ``forward`` / ``backward`` are the same two calls for code that drives a Function's static
    methods itself -- through the ``fn2`` operators while ``torch.compile`` traces, which is how it sees ``apply``."""

    @classmethod
    def apply(cls, coords, radius, *pyramid):
        return corr_sample_cuda.apply(list(pyramid), coords, radius)

    @staticmethod
    def forward(ctx, coords, radius, *pyramid):
        ctx.save_for_backward(coords, *pyramid)
        ctx.radius = radius
        if torch.compiler.is_compiling():
            _no_coords_gradient(ctx.needs_input_grad[0])
            return _forward_op(list(pyramid), coords, radius)
        return corr_sample_cuda.forward_alloc(list(pyramid), coords, radius)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        coords, *pyramid = ctx.saved_tensors
        if torch.compiler.is_compiling():
            grads = _backward_op(pyramid, coords, grad_output, ctx.radius)
        else:
            grads = corr_sample_cuda.backward_alloc(pyramid, coords, grad_output, ctx.radius)
        return (None, None, *grads)


def corr_sample(pyramid, coords, radius):
    """The lookup of ``pyramid`` (a sequence of (B H W) x 1 x H2_l x W2_l float32 levels) at ``coords`` (B x 2 x H x W, level-0
    cells): B x (len(pyramid) (2 radius + 1)^2) x H x W.  Differentiable in the levels."""
    return CorrSampleFunction.apply(coords, radius, *pyramid)


class CorrSample(nn.Module):
    """``CorrSample(radius)(pyramid, coords)`` -> B x (L (2 radius + 1)^2) x H x W."""

    def __init__(self, radius):
        super().__init__()
        self.radius = radius

    def forward(self, pyramid, coords):
        return corr_sample(pyramid, coords, self.radius)

    def extra_repr(self):
        return f"radius={self.radius}"


class CorrBlock:
    """The constructor and call of RAFT's ``CorrBlock`` (``core/corr.py``; ``raft.py`` with ``alternate_corr=False``): the all-pairs
    volume fmap1^T fmap2 / sqrt(C) of the ``.float()`` maps, reshaped to (B H W, 1, H, W), average-pooled once per further level;
    every call samples all levels at ``coords / 2**level`` in one kernel: B x (num_levels * (2 radius + 1)^2) x H x W float32.
    ``coords`` is used detached, as RAFT passes it.  ``fused_build=True`` (opt-in, incubating) builds the pyramid with
    ``corr_pyramid`` (corr_pyramid.py) instead: one fused MFMA kernel in place of the matmul, the scale and the pooling passes, the
    same levels within the bound of include/preview/flownet2_hip_pyramid.h."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, fused_build=False):
        self.num_levels = num_levels
        self.radius = radius
        fmap1, fmap2 = fmap1.float(), fmap2.float()
        if fused_build:
            from ._fused_build import build_pyramid   # corr_pyramid.corr_pyramid; loads corr_pyramid_cuda, only where it is asked for
            self.corr_pyramid = build_pyramid(fmap1.contiguous(), fmap2.contiguous(), num_levels)
            return
        B, C, H, W = fmap1.shape
        H2, W2 = fmap2.shape[2:]
        corr = torch.matmul(fmap1.reshape(B, C, H * W).transpose(1, 2), fmap2.reshape(B, C, H2 * W2)) / math.sqrt(C)
        corr = corr.reshape(B * H * W, 1, H2, W2)
        self.corr_pyramid = [corr]
        for _ in range(num_levels - 1):
            corr = F.avg_pool2d(corr, 2, stride=2)
            self.corr_pyramid.append(corr)

    def __call__(self, coords):
        return corr_sample(self.corr_pyramid, coords.detach().float(), self.radius)
