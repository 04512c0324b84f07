"""ForwardWarp: forward flow splatting -- every source pixel is moved along its flow and added bilinearly onto the four pixels
around where it lands -- as an autograd Function + Module over the ``forward_warp_cuda`` extension
(csrc/binding/forward_warp_cuda.cpp, csrc/forward_warp.hip), with the compositions built on it: ``softsplat`` (summation,
average, linear and softmax splatting) and ``range_map`` (how much lands on every pixel; UnFlow's occlusion estimate).

    out[n, c, y0 + dy, x0 + dx] += w_dydx * input[n, c, y, x],    (x0, y0) = floor((x, y) + flow[n, :, y, x]), bilinear w

``input`` is float32 N x C x H x W, ``flow`` float32 N x 2 x H x W (channel 0 = x, 1 = y); the output has the input's size, a
pixel that lands outside (or on NaN / inf) adds nothing.  Both inputs get gradients; the backward is a gather without atomics and
bit-reproducible.  The forward adds with float atomics, so its last bits may differ from run to run; under
``torch.use_deterministic_algorithms(True)`` it sums in fixed point instead and is bit-reproducible too.  Semantics, arithmetic
order and bounds are documented in include/flownet2_hip_splat.h.  Importing this module fails loudly if the extension has not
been built: the HIP kernels are the only implementation.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import forward_warp_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose


class ForwardWarpFunction(Function):
    """``apply`` goes straight to the autograd node the extension implements in C++ (``forward_warp_cuda.apply``);
    ``forward`` / ``backward`` are the same two calls for code that drives a Function's static methods itself."""

    @classmethod
    def apply(cls, input, flow):
        return forward_warp_cuda.apply(input, flow)

    @staticmethod
    def forward(ctx, input, flow):
        ctx.save_for_backward(input, flow)
        return forward_warp_cuda.forward_alloc(input, flow)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, flow = ctx.saved_tensors
        want_input, want_flow = ctx.needs_input_grad[:2]
        if not (want_input or want_flow):
            return None, None
        return tuple(forward_warp_cuda.backward_alloc(input, flow, grad_output, want_input, want_flow))


class ForwardWarp(nn.Module):
    """``ForwardWarp()(input, flow)`` -> N x C x H x W: the summation splat of ``input`` along ``flow``."""

    def forward(self, input, flow):
        return ForwardWarpFunction.apply(input, flow)


SOFTSPLAT_EPS = 1e-7


def softsplat(input, flow, metric=None, mode="sum"):
    """Softmax splatting (Niklaus and Liu, CVPR 2020) as compositions over ``ForwardWarpFunction``; S = the summation splat.

        sum     S(input)
        avg     S(input) / (S(1) + 1e-7)                                     one splat of cat([input, 1])
        linear  S(input * metric) / (S(metric) + 1e-7)                       one splat of cat([input * metric, metric])
        soft    S(input * exp(metric)) / (S(exp(metric)) + 1e-7)             ``linear`` with exp(metric) in place of metric

    ``metric`` is N x 1 x H x W and required by ``linear`` and ``soft`` (and refused by the other two); the weighting and the
    division are PyTorch operations, differentiable in ``input``, ``flow`` and ``metric``."""
    if mode not in ("sum", "avg", "linear", "soft"):
        raise ValueError(f"softsplat: mode {mode!r} is not one of 'sum', 'avg', 'linear', 'soft'")
    if (metric is not None) != (mode in ("linear", "soft")):
        raise ValueError(f"softsplat: mode {mode!r} " + ("needs a metric of shape N x 1 x H x W" if metric is None else
                                                         "takes no metric: pass metric=None or use mode 'linear' or 'soft'"))
    if mode == "sum":
        return ForwardWarpFunction.apply(input, flow)
    if mode == "avg":
        weight = input.new_ones((input.shape[0], 1) + tuple(input.shape[2:]))
        stacked = torch.cat([input, weight], 1)
    else:
        if metric.dim() != 4 or metric.shape[1] != 1 or metric.shape[0] != input.shape[0] or metric.shape[2:] != input.shape[2:]:
            raise ValueError(f"softsplat: metric of shape {tuple(metric.shape)} must be N x 1 x H x W for input {tuple(input.shape)}")
        weight = metric.exp() if mode == "soft" else metric
        stacked = torch.cat([input * weight, weight], 1)
    out = ForwardWarpFunction.apply(stacked, flow)
    return out[:, :-1] / (out[:, -1:] + SOFTSPLAT_EPS)


def range_map(flow):
    """The splat of ones along ``flow``, N x 1 x H x W: how much of the source lands on every pixel.  Values near 0 mark pixels
    nothing maps to (occluded in the other frame, as UnFlow / DDFlow / SMURF use it)."""
    if flow.dim() != 4:
        raise ValueError(f"range_map: flow of shape {tuple(flow.shape)} must be N x 2 x H x W")
    return ForwardWarpFunction.apply(flow.new_ones((flow.shape[0], 1) + tuple(flow.shape[2:])), flow)
