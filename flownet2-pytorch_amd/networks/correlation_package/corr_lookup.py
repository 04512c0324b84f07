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


class CorrLookupFunction(Function):
    """``apply`` goes straight to the autograd node the extension implements in C++ (``corr_lookup_cuda.apply``); ``forward`` /
    ``backward`` are the same two calls for code that drives a Function's static methods itself."""

    @classmethod
    def apply(cls, fmap1, fmap2, coords, radius, scale):
        return corr_lookup_cuda.apply(fmap1, fmap2, coords, radius, scale)

    @staticmethod
    def forward(ctx, fmap1, fmap2, coords, radius, scale):
        ctx.save_for_backward(fmap1, fmap2, coords)
        ctx.lookup_params = (radius, scale)
        return corr_lookup_cuda.forward_alloc(fmap1, fmap2, coords, radius, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        fmap1, fmap2, coords = ctx.saved_tensors
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
