"""CorrSample1d and CorrBlock1D (staging): the lookup of a PREBUILT 1-D correlation pyramid -- RAFT-Stereo's default ``CorrBlock1D``
(``core/corr.py``, its ``reg`` implementation) and that of the stereo networks built on it -- autograd Function + Module over the
``corr_sample1d_cuda`` extension (csrc/binding/corr_sample1d_cuda.cpp, csrc/corr_sample1d.hip).

    out[n, l*D + i, y, x] = w0 * level_l[(n*H + y)*W + x, 0, 0, x0 + i - r] + w1 * level_l[(n*H + y)*W + x, 0, 0, x0 + i - r + 1]

with x0 = floor(coords[n, 0, y, x] / 2**l), D = 2 r + 1 and the linear weights w0 = 1 - fx, w1 = fx of the fractional part: one
kernel in place of RAFT-Stereo's ``linspace``, ``grid_sample`` and ``view`` per level, ``cat``, ``permute`` and ``float``, and a
backward that writes the levels' gradients without atomics, bit-reproducibly.  The row-wise ``einsum`` and the ``avg_pool2d`` pyramid
stay in PyTorch (rocBLAS / MIOpen): they run once per step.  ``coords`` is RAFT-Stereo's B x 2 x H x W tensor, of which only channel
0 (x, in level-0 cells) is read -- in place, without a copy -- or a B x 1 x H x W tensor; it gets no gradient and must not require
one.  float32 only.  Semantics, bounds and the checks are documented in include/staging/flownet2_hip_sample1d.h.  Importing this
module fails loudly if the extension has not been built: the HIP kernels are the only implementation.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import corr_sample1d_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose
import fn2_ops
from fn2_ops import refuse

MAX_RADIUS = 8   # FN2H_MAX_RADIUS (include/staging/flownet2_hip_sample1d.h)
MAX_LEVELS = 8   # FN2H_MAX_LEVELS


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _fake_coords(coords, levels, radius, op):
    """check_coords of csrc/binding/corr_sample1d_cuda.cpp, as far as shapes and dtypes decide it."""
    refuse(coords.dtype == torch.float32, op, ": coords must be float32, got ", coords.dtype, ": convert it with .float()")
    refuse(1 <= levels <= MAX_LEVELS, op, ": the pyramid has ", levels, " levels, expected 1 .. ", MAX_LEVELS)
    refuse(0 <= radius <= MAX_RADIUS, op, ": radius ", radius, " outside 0 .. ", MAX_RADIUS)
    refuse(coords.dim() == 4 and (coords.shape[1] == 1 or coords.shape[1] == 2), op, ": coords has shape ", tuple(coords.shape),
           ", expected [B, 2, H, W] (RAFT-Stereo's; channel 0 is read) or [B, 1, H, W]")
    return coords.shape[0] * coords.shape[2] * coords.shape[3]


def _forward_fake(pyramid, coords, radius):
    op = "fn2::corr_sample1d"
    pixels = _fake_coords(coords, len(pyramid), radius, op)
    for lvl in pyramid:
        refuse(lvl.dtype == torch.float32, op, ": float32 tensors expected, got ", lvl.dtype,
               " (RAFT-Stereo builds its correlation volume in float: use .float())")
        refuse(((lvl.dim() == 4 and lvl.shape[1] == 1 and lvl.shape[2] == 1) or lvl.dim() == 2) and lvl.shape[0] == pixels, op,
               ": a pyramid level has shape ", tuple(lvl.shape), ", expected [", pixels, ", 1, 1, W2] or [", pixels, ", W2] for coords ",
               tuple(coords.shape))
    return coords.new_empty((coords.shape[0], len(pyramid) * (2 * radius + 1), coords.shape[2], coords.shape[3]))


def _backward_fake(coords, grad_output, widths, dims, radius):
    op = "fn2::corr_sample1d_backward"
    pixels = _fake_coords(coords, len(widths), radius, op)
    refuse(len(dims) == len(widths), op, ": ", len(widths), " widths but ", len(dims), " dims")
    D = 2 * radius + 1
    refuse(grad_output.dim() == 4 and grad_output.shape[0] == coords.shape[0] and grad_output.shape[1] == len(widths) * D
           and grad_output.shape[2] == coords.shape[2] and grad_output.shape[3] == coords.shape[3], op,
           ": gradOutput has shape ", tuple(grad_output.shape), ", expected [", coords.shape[0], ", ", len(widths) * D, ", ", coords.shape[2],
           ", ", coords.shape[3], "]")
    for l, (w, d) in enumerate(zip(widths, dims)):
        refuse(d == 2 or d == 4, op, ": level ", l, " has ", d, " dimensions, expected 2 ([P, W2]) or 4 ([P, 1, 1, W2])")
        refuse(w >= 1, op, ": level ", l, " is ", w, " cells wide, expected at least 1")
    return [coords.new_empty((pixels, 1, 1, w) if d == 4 else (pixels, w)) for w, d in zip(widths, dims)]


def _no_coords_gradient(wanted):
    # a silent None for coords would train wrongly: RAFT-Stereo detaches coords in every iteration, and so must the caller
    if wanted:
        raise RuntimeError("CorrSample1d: coords requires grad, but this layer has no gradient for coords (as RAFT-Stereo's sampler): "
                           "pass coords.detach()")


def _shapes(pyramid):
    """What the backward needs of the levels: their widths and whether each is [P, 1, 1, W2] or [P, W2].  The levels themselves are
    not saved for it: it reads none of them, and a pyramid is hundreds of megabytes."""
    return [t.shape[-1] for t in pyramid], [t.dim() for t in pyramid]


def _setup(ctx, inputs, output):
    pyramid, coords, radius = inputs
    _no_coords_gradient(ctx.needs_input_grad[-2])   # (from the end: the flags of a Tensor[] argument may come flattened)
    ctx.save_for_backward(coords)
    ctx.widths, ctx.dims = _shapes(pyramid)
    ctx.radius = radius


def _grad(ctx, grad_output):
    coords, = ctx.saved_tensors
    return _backward_op(coords, grad_output, ctx.widths, ctx.dims, ctx.radius), None, None


_forward_op = fn2_ops.define("corr_sample1d", "(Tensor[] pyramid, Tensor coords, int radius) -> Tensor",
                             corr_sample1d_cuda.forward_alloc, _forward_fake, _grad, _setup, staging=True)
_backward_op = fn2_ops.define("corr_sample1d_backward",
                              "(Tensor coords, Tensor grad_output, SymInt[] widths, int[] dims, int radius) -> Tensor[]",
                              corr_sample1d_cuda.backward_alloc, _backward_fake, staging=True)


class CorrSample1dFunction(Function):
    """``apply(coords, radius, *pyramid)`` goes straight to the autograd node the extension implements in C++
    (``corr_sample1d_cuda.apply``); ``forward`` / ``backward`` are the same two calls for code that drives a Function's static
    methods itself -- through the ``fn2`` operators while ``torch.compile`` traces, which is how it sees ``apply``."""

    @classmethod
    def apply(cls, coords, radius, *pyramid):
        return corr_sample1d_cuda.apply(list(pyramid), coords, radius)

    @staticmethod
    def forward(ctx, coords, radius, *pyramid):
        _no_coords_gradient(ctx.needs_input_grad[0])
        ctx.save_for_backward(coords)
        ctx.widths, ctx.dims = _shapes(pyramid)
        ctx.radius = radius
        if torch.compiler.is_compiling():
            return _forward_op(list(pyramid), coords, radius)
        return corr_sample1d_cuda.forward_alloc(list(pyramid), coords, radius)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        coords, = ctx.saved_tensors
        if torch.compiler.is_compiling():
            grads = _backward_op(coords, grad_output, ctx.widths, ctx.dims, ctx.radius)
        else:
            grads = corr_sample1d_cuda.backward_alloc(coords, grad_output, ctx.widths, ctx.dims, ctx.radius)
        return (None, None, *grads)


def corr_sample1d(pyramid, coords, radius):
    """The lookup of ``pyramid`` (a sequence of (B H W) x 1 x 1 x W2_l float32 levels) at ``coords`` (B x 2 x H x W, channel 0 = x in
    level-0 cells, or B x 1 x H x W): B x (len(pyramid) (2 radius + 1)) x H x W.  Differentiable in the levels."""
    return CorrSample1dFunction.apply(coords, radius, *pyramid)


class CorrSample1d(nn.Module):
    """``CorrSample1d(radius)(pyramid, coords)`` -> B x (L (2 radius + 1)) x H x W."""

    def __init__(self, radius):
        super().__init__()
        self.radius = radius

    def forward(self, pyramid, coords):
        return corr_sample1d(pyramid, coords, self.radius)

    def extra_repr(self):
        return f"radius={self.radius}"


class CorrBlock1D:
    """The constructor and call of RAFT-Stereo's ``CorrBlock1D`` (``core/corr.py``): the row-wise volume
    ``einsum('aijk,aijh->ajkh', fmap1, fmap2) / sqrt(C)`` of the ``.float()`` maps, reshaped to (B H W1, 1, 1, W2), average-pooled
    along its last axis once per further level; every call samples all levels at ``coords[:, :1] / 2**level`` in one kernel:
    B x (num_levels * (2 radius + 1)) x H x W1 float32.  ``coords`` is used detached, as RAFT-Stereo passes it.  ``num_levels``
    levels are kept (RAFT-Stereo pools once more and never reads the result); a level that would be empty is a ``ValueError``."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        self.num_levels = num_levels
        self.radius = radius
        fmap1, fmap2 = fmap1.float(), fmap2.float()
        B, C, H, W1 = fmap1.shape
        W2 = fmap2.shape[3]
        if num_levels < 1 or W2 >> (num_levels - 1) < 1:
            raise ValueError(f"CorrBlock1D: num_levels {num_levels} leaves an empty level for fmap2 of width {W2}: "
                             f"use at most {max(W2, 1).bit_length()} levels")
        corr = torch.einsum("aijk,aijh->ajkh", fmap1, fmap2) / math.sqrt(C)
        corr = corr.reshape(B * H * W1, 1, 1, W2)
        self.corr_pyramid = [corr]
        for _ in range(num_levels - 1):
            corr = F.avg_pool2d(corr, [1, 2], stride=[1, 2])
            self.corr_pyramid.append(corr)

    def __call__(self, coords):
        return corr_sample1d(self.corr_pyramid, coords.detach().float(), self.radius)
