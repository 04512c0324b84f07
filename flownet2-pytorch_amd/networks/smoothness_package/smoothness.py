"""The edge-aware smoothness regulariser of first or second order, the third term of unsupervised optical flow (UnFlow, ARFlow,
UFlow, SMURF), as an autograd Function + Modules over the ``smoothness_cuda`` extension (csrc/binding/smoothness_cuda.cpp,
csrc/smooth.hip).

    w = exp(-mean_c |alpha dI_c|)  (exponential)    or    exp(-mean_c (alpha dI_c)^2)  (gaussian),    dI_c = I_c[p + k] - I_c[p]
    out[n, 0 or 1, p] = w sum_f sqrt(d_f^2 + eps^2),    d_f the first (order 1) or second (order 2) difference of the flow in x or y

``flow`` is float32 N x F x H x W with F = 1 .. 4, ``image`` float32 N x C x H x W with C = 1 or 3; the result is N x 2 x H x W,
plane 0 the x term and plane 1 the y term, exactly 0 where the stencil does not fit (the last k columns / rows).  The flow gets a
gradient -- a gather without atomics, bit-reproducible -- the image does not: an image that requires one is refused.  One kernel
each way replaces about twenty elementwise launches and their full-size temporaries.  Semantics, arithmetic order and bounds are
documented in include/flownet2_hip_smooth.h.
Importing this module fails loudly if the extension has not been built: the HIP kernels are the only implementation.
"""
import math

from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import smoothness_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose

EDGE_WEIGHTINGS = {"exponential": smoothness_cuda.EDGE_EXPONENTIAL, "gaussian": smoothness_cuda.EDGE_GAUSSIAN}


def _options(order, edge_weighting, alpha, eps, who):
    """(order, edge code, alpha, eps) or ValueError: the same checks for the function and the modules' constructors."""
    if order not in (1, 2):
        raise ValueError(f"{who}: order {order!r} is not 1 or 2")
    if edge_weighting not in EDGE_WEIGHTINGS:
        raise ValueError(f"{who}: edge_weighting {edge_weighting!r} is not 'exponential' or 'gaussian'")
    for name, v in (("alpha", alpha), ("eps", eps)):
        if not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{who}: {name} {v!r} is not a finite number >= 0")
    return int(order), EDGE_WEIGHTINGS[edge_weighting], float(alpha), float(eps)


class SmoothnessFunction(Function):
    """``apply`` goes straight to the autograd node the extension implements in C++ (``smoothness_cuda.apply``);
    ``forward`` / ``backward`` are the same two calls for code that drives a Function's static methods itself."""

    @classmethod
    def apply(cls, flow, image, order=1, edge_weighting="exponential", alpha=150.0, eps=0.001):
        return smoothness_cuda.apply(flow, image, *_options(order, edge_weighting, alpha, eps, "SmoothnessFunction"))

    @staticmethod
    def forward(ctx, flow, image, order=1, edge_weighting="exponential", alpha=150.0, eps=0.001):
        ctx.options = _options(order, edge_weighting, alpha, eps, "SmoothnessFunction")
        ctx.save_for_backward(flow, image)
        return smoothness_cuda.forward_alloc(flow, image, *ctx.options)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        flow, image = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            raise RuntimeError("SmoothnessFunction: image requires a gradient, and this layer has none for the image: pass image.detach()")
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        return smoothness_cuda.backward_alloc(flow, image, grad_output, *ctx.options), None, None, None, None, None


def smoothness_map(flow, image, order=1, edge_weighting="exponential", alpha=150.0, eps=0.001):
    """N x 2 x H x W: the edge-weighted robust flow differences in x (plane 0) and y (plane 1)."""
    return SmoothnessFunction.apply(flow, image, order, edge_weighting, alpha, eps)


class EdgeAwareSmoothness(nn.Module):
    """``EdgeAwareSmoothness(order=2)(flow, image)`` -> N x 2 x H x W, ``smoothness_map`` with the parameters kept in the module."""

    def __init__(self, order=1, edge_weighting="exponential", alpha=150.0, eps=0.001):
        super().__init__()
        _options(order, edge_weighting, alpha, eps, type(self).__name__)
        self.order, self.edge_weighting, self.alpha, self.eps = int(order), edge_weighting, float(alpha), float(eps)

    def forward(self, flow, image):
        return SmoothnessFunction.apply(flow, image, self.order, self.edge_weighting, self.alpha, self.eps)

    def extra_repr(self):
        return f"order={self.order}, edge_weighting={self.edge_weighting!r}, alpha={self.alpha}, eps={self.eps}"


class SmoothnessLoss(EdgeAwareSmoothness):
    """UFlow's smoothness loss: ``loss(flow, image)`` ->

        ( sum(out[:, 0]) / (N F H (W - k))  +  sum(out[:, 1]) / (N F (H - k) W) ) / 2

    the mean over every flow-gradient element per direction; a direction with no valid cell (W <= k or H <= k) counts as 0.  The
    two planes are the HIP kernel; the two sums act on them and stay in PyTorch."""

    def forward(self, flow, image):
        out = super().forward(flow, image)
        N, F, H, W = flow.shape
        k = self.order
        nx, ny = N * F * H * (W - k), N * F * (H - k) * W
        lx = out[:, 0].sum() / nx if nx > 0 else out[:, 0].sum() * 0.0
        ly = out[:, 1].sum() / ny if ny > 0 else out[:, 1].sum() * 0.0
        return (lx + ly) / 2
