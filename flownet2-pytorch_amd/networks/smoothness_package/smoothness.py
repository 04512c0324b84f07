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

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import smoothness_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose

import fn2_ops
from fn2_ops import refuse

EDGE_WEIGHTINGS = {"exponential": smoothness_cuda.EDGE_EXPONENTIAL, "gaussian": smoothness_cuda.EDGE_GAUSSIAN}
_FLT_MAX = 3.4028234663852886e38


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _fake_inputs(flow, image, order, edge, alpha, eps, op):
    """check_inputs of csrc/binding/smoothness_cuda.cpp, as far as shapes, dtypes and parameters decide it."""
    refuse(flow.dim() == 4 and image.dim() == 4, op, ": flow and image must be 4-D (N, channels, H, W); add the missing dimensions with [None]")
    refuse(flow.shape[0] == image.shape[0] and flow.shape[2] == image.shape[2] and flow.shape[3] == image.shape[3], op, ": image ",
           tuple(image.shape), " must have the batch, height and width of flow ", tuple(flow.shape))
    refuse(1 <= flow.shape[1] <= smoothness_cuda.MAX_FLOW_CHANNELS, op, ": flow has ", flow.shape[1], " channels, expected 1 to 4")
    refuse(image.shape[1] == 1 or image.shape[1] == 3, op, ": the image has ", image.shape[1], " channels, expected 1 (grey) or 3 (RGB)")
    refuse(order in (1, 2), op, ": order ", order, " is not 1 or 2")
    refuse(edge in EDGE_WEIGHTINGS.values(), op, ": edge_weighting ", edge, " is not 0 (exponential) or 1 (gaussian)")
    refuse(0 <= alpha <= _FLT_MAX, op, ": alpha ", alpha, " is not a finite float >= 0")
    refuse(0 <= eps <= _FLT_MAX, op, ": eps ", eps, " is not a finite float >= 0")
    for name, t in (("flow", flow), ("image", image)):
        refuse(t.dtype == torch.float32, op, ": ", name, " must be float32, got ", t.dtype, ": convert it with .float()")


def _forward_fake(flow, image, order, edge, alpha, eps):
    _fake_inputs(flow, image, order, edge, alpha, eps, "fn2::smoothness")
    return flow.new_empty((flow.shape[0], 2, flow.shape[2], flow.shape[3]))


def _backward_fake(flow, image, grad_output, order, edge, alpha, eps):
    _fake_inputs(flow, image, order, edge, alpha, eps, "fn2::smoothness_backward")
    return flow.new_empty(flow.shape)


def _no_image_gradient(wanted):
    if wanted:
        raise RuntimeError("SmoothnessFunction: image requires a gradient, and this layer has none for the image: pass image.detach()")


def _setup(ctx, inputs, output):
    _no_image_gradient(ctx.needs_input_grad[1])
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.options = tuple(inputs[2:])


def _grad(ctx, grad_output):
    flow, image = ctx.saved_tensors
    if not ctx.needs_input_grad[0]:
        return None, None, None, None, None, None
    return _backward_op(flow, image, grad_output, *ctx.options), None, None, None, None, None


_forward_op = fn2_ops.define("smoothness", "(Tensor flow, Tensor image, int order, int edge_weighting, float alpha, float eps) -> Tensor",
                             smoothness_cuda.forward_alloc, _forward_fake, _grad, _setup)
_backward_op = fn2_ops.define(
    "smoothness_backward", "(Tensor flow, Tensor image, Tensor grad_output, int order, int edge_weighting, float alpha, float eps) -> Tensor",
    smoothness_cuda.backward_alloc, _backward_fake)


def _options(order, edge_weighting, alpha, eps, who):
    """(order, edge code, alpha, eps) or ValueError: the same checks for the function and the modules' constructors."""
    if order not in (1, 2):
        raise ValueError(f"{who}: order {order!r} is not 1 or 2")
    if edge_weighting not in EDGE_WEIGHTINGS:
        raise ValueError(f"{who}: edge_weighting {edge_weighting!r} is not 'exponential' or 'gaussian'")
    for name, v in (("alpha", alpha), ("eps", eps)):
        if not isinstance(v, (int, float)) or not 0 <= v < math.inf:   # (comparisons: a traced, symbolic float passes through them)
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
        if torch.compiler.is_compiling():   # Dynamo traces apply() through this method: the operator it can see
            _no_image_gradient(ctx.needs_input_grad[1])   # (eager: smoothness_cuda.apply refuses it before the node)
            return _forward_op(flow, image, *ctx.options)
        return smoothness_cuda.forward_alloc(flow, image, *ctx.options)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        flow, image = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            raise RuntimeError("SmoothnessFunction: image requires a gradient, and this layer has none for the image: pass image.detach()")
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        backward_alloc = _backward_op if torch.compiler.is_compiling() else smoothness_cuda.backward_alloc
        return backward_alloc(flow, image, grad_output, *ctx.options), None, None, None, None, None


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
