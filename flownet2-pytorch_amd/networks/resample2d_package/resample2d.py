"""Resample2d (flow warp): autograd Function + Module over the ``resample2d_cuda`` extension.

Same public names and signatures as the reference wrapper
(networks/resample2d_package/resample2d.py:5-49): ``Resample2dFunction.apply(input1, input2,
kernel_size, bilinear)`` and ``Resample2d(kernel_size=1, bilinear=True)``; output shape is
(B, C_img, H, W) with B, H, W taken from the flow (reference :16-18).  float32, as in the
reference; bfloat16 tensors (autocast) are widened to float32 around the float32 kernels and each
result is rounded to bfloat16 once (Resample2d refuses half, as the reference does).  The fused rows
WarpDiffNormCat / WarpDiffNorm take half and bfloat16 tensors natively: 16-bit kernels with the float32
arithmetic inside, bit-identical to the widened float32 call rounded once.  Unlike the reference Module (:48) the image is NOT made contiguous first: the HIP
kernel honours input1's strides, which saves a full copy of the channel slice models.py:133
passes in.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import resample2d_cuda  # built by flownet2-pytorch_amd/build.py; no fallback on purpose

_LOWP = (torch.float16, torch.bfloat16)   # the fused rows' native 16-bit element types


class Resample2dFunction(Function):
    """``apply`` = the C++ autograd node ``resample2d_cuda.apply`` (no Python between ``apply`` and the launch, no GIL in the backward);
    ``forward`` / ``backward`` are the same two calls in Python for code written against the reference's static methods."""

    @classmethod
    def apply(cls, input1, input2, kernel_size=1, bilinear=True):
        assert input2.is_contiguous(), "flow must be contiguous (reference resample2d.py:10)"
        if int(kernel_size) < 1:
            raise ValueError("Resample2d: kernel_size must be >= 1")
        return resample2d_cuda.apply(input1, input2, int(kernel_size), bool(bilinear))

    @staticmethod
    def forward(ctx, input1, input2, kernel_size=1, bilinear=True):
        assert input2.is_contiguous(), "flow must be contiguous (reference resample2d.py:10)"
        ctx.save_for_backward(input1, input2)
        ctx.kernel_size, ctx.bilinear = kernel_size, bilinear
        if int(kernel_size) < 1:
            raise ValueError("Resample2d: kernel_size must be >= 1")
        # output: (B, C_img, H, W) with B, H, W from the flow (reference :16-18), allocated on the C++ side and fully written
        return resample2d_cuda.forward_alloc(input1, input2, kernel_size, bilinear)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
        # grad_input1 is accumulated into by the kernel (fp32 atomics), so it starts at zero (reference resample2d.py:31): zeros and the
        # contiguous copy of grad_output are made on the C++ side.  (Folding the fill into the kernel was built and measured in round 5:
        # slower than this fill)
        grad_input1, grad_input2 = resample2d_cuda.backward_alloc(input1, input2, grad_output, ctx.kernel_size, ctx.bilinear)
        return grad_input1, grad_input2, None, None


class Resample2d(nn.Module):
    def __init__(self, kernel_size=1, bilinear=True):
        super().__init__()
        # kernel_size > 1: window sums as in resample2d_kernel.cu:54-61 with the shifted indices clamped to the image (the
        # reference reads past its tensors there); FlowNet2 itself only uses 1 (models.py:48,51)
        if int(kernel_size) < 1:
            raise ValueError("Resample2d: kernel_size must be >= 1")
        self.kernel_size = kernel_size
        self.bilinear = bilinear

    def forward(self, input1, input2):
        return Resample2dFunction.apply(input1, input2, self.kernel_size, self.bilinear)


class WarpDiffNormCatFunction(Function):
    """models.py:133-138 as one differentiable op: forward = fn2_warp_diff_norm_cat, backward = fn2_warp_diff_norm_cat_backward
    (the gradient through resample -> difference -> ChannelNorm -> cat in one kernel; no scatter at all when the image pair
    needs no gradient, which is the case in FlowNet2, where it is the network's input).  ``apply`` = the C++ autograd node
    ``resample2d_cuda.warp_diff_norm_cat_apply``."""

    @classmethod
    def apply(cls, x, flow, div_flow, bilinear):
        return resample2d_cuda.warp_diff_norm_cat_apply(x, flow, float(div_flow), bool(bilinear))

    # Element types, as the C++ node: x and flow of the same 16-bit type and no gradient for x -> the native 16-bit kernels (the backward
    # recomputes warp and norm: the output is not saved); a 16-bit x that needs a gradient, or mixed types -> widened around the
    # float32 kernels, each result rounded once
    @staticmethod
    def forward(ctx, x, flow, div_flow, bilinear):
        ctx.types = (x.dtype, flow.dtype)
        native16 = x.dtype == flow.dtype and x.dtype in _LOWP and not ctx.needs_input_grad[0]
        if not native16 and (x.dtype in _LOWP or x.dtype != flow.dtype):
            x, flow = x.float(), flow.float()
        x, flow = x.contiguous(), flow.contiguous()
        b, c2, h, w = x.shape
        out = x.new_empty((b, c2 + c2 // 2 + 3, h, w))
        resample2d_cuda.warp_diff_norm_cat(x, flow, out, float(div_flow), bool(bilinear))
        ctx.save_for_backward(*((x, flow) if native16 else (x, flow, out)))
        ctx.div_flow, ctx.bilinear = float(div_flow), bool(bilinear)
        return out.to(ctx.types[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, flow = ctx.saved_tensors[:2]
        out = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else x.new_empty(0)
        need_x, need_flow = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_flow):
            return None, None, None, None
        grad_x = torch.empty_like(x) if need_x else x.new_empty(0)
        grad_flow = torch.empty_like(flow)
        resample2d_cuda.warp_diff_norm_cat_backward(x, flow, out, grad_out.to(x.dtype).contiguous(), grad_x, grad_flow, ctx.div_flow, ctx.bilinear)
        return (grad_x.to(ctx.types[0]) if need_x else None), (grad_flow.to(ctx.types[1]) if need_flow else None), None, None


class WarpDiffNormCat(nn.Module):
    """the five statements models.py:133-138 --

        resampled = Resample2d()(x[:, 3:], flow);  diff = x[:, :3] - resampled;  norm = ChannelNorm()(diff)
        concat = torch.cat((x, resampled, flow / div_flow, norm), dim=1)

    -- as one kernel pass (the reference makes x[:, 3:] contiguous, writes and re-reads the warped image, the difference
    and the norm, then copies all twelve channels again for the concat), differentiable (WarpDiffNormCatFunction): one
    backward kernel instead of cat / div / ChannelNorm / sub / Resample2d backward passes and their zero fills."""

    def __init__(self, div_flow=20.0, bilinear=True):
        super().__init__()
        self.div_flow = div_flow
        self.bilinear = bilinear

    def forward(self, x, flow):
        return WarpDiffNormCatFunction.apply(x, flow, float(self.div_flow), self.bilinear)


class WarpDiffNormFunction(Function):
    """models.py:157-161 / :170-174 as one differentiable op: ``ChannelNorm(x[:, :3] - Resample2d(x[:, 3:], flow))``.  Forward = the fused
    kernel storing only the norm plane; backward w.r.t. the flow = one gather-only kernel that recomputes the warp
    (fn2_warp_diff_norm_backward).  When the image pair itself needs a gradient the unfused layers are composed under autograd.
    ``apply`` = the C++ autograd node ``resample2d_cuda.warp_diff_norm_apply``."""

    @classmethod
    def apply(cls, x, flow, bilinear):
        return resample2d_cuda.warp_diff_norm_apply(x, flow, bool(bilinear))

    @staticmethod
    def forward(ctx, x, flow, bilinear):
        ctx.types = (x.dtype, flow.dtype)
        native16 = x.dtype == flow.dtype and x.dtype in _LOWP
        if x.dtype != flow.dtype:   # mixed types: widened around the float32 kernels
            x, flow = x.float(), flow.float()
        x, flow = x.contiguous(), flow.contiguous()
        norm = resample2d_cuda.warp_diff_norm(x, flow, bool(bilinear))
        ctx.save_for_backward(*((x, flow) if native16 else (x, flow, norm)))   # the 16-bit backward recomputes the norm
        ctx.bilinear = bool(bilinear)
        return norm.to(ctx.types[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_norm):
        if not ctx.needs_input_grad[1]:
            return None, None, None
        x, flow = ctx.saved_tensors[:2]
        norm = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else x.new_empty(0)
        grad_flow = resample2d_cuda.warp_diff_norm_backward(x, flow, norm, grad_norm.to(x.dtype).contiguous(), ctx.bilinear)
        return None, grad_flow.to(ctx.types[1]), None


class WarpDiffNorm(nn.Module):
    """``||x[:, :C] - warp(x[:, C:], flow)||_2`` (B x 1 x H x W): the brightness error FlowNet2 feeds its fusion network
    (models.py:157-161, :170-174) in one kernel pass instead of Resample2d + subtraction + ChannelNorm."""

    def __init__(self, bilinear=True):
        super().__init__()
        self.bilinear = bilinear

    def forward(self, x, flow):
        if x.requires_grad and torch.is_grad_enabled():
            # the pair itself wants a gradient (not the case in FlowNet2, where it is the input): the unfused layers under autograd
            from networks.channelnorm_package.channelnorm import ChannelNormFunction
            if x.dtype in _LOWP:   # Resample2d is float32 (and refuses half): widened first, the result rounded once
                return self.forward(x.float(), flow.float()).to(x.dtype)
            c = x.shape[1] // 2
            # (flow made contiguous like the fused path does: the same module must not accept a strided flow or raise depending on
            # whether the pair wants a gradient -- ADVICE r5)
            return ChannelNormFunction.apply(x[:, :c] - Resample2dFunction.apply(x[:, c:], flow.contiguous(), 1, self.bilinear), 2)
        return WarpDiffNormFunction.apply(x, flow, self.bilinear)
