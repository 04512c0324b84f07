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

import fn2_ops
from fn2_ops import refuse

_LOWP = (torch.float16, torch.bfloat16)   # the fused rows' native 16-bit element types
_WARP_DTYPES = (torch.float32,) + _LOWP


# ---- the fn2 operators (fn2_ops.py): the same binding calls as the static methods below, for torch.compile
def _resample2d(input1, input2, kernel_size, bilinear):
    refuse(input2.is_contiguous(), "Resample2dFunction: flow must be contiguous (reference resample2d.py:10)")
    return resample2d_cuda.forward_alloc(input1, input2, kernel_size, bilinear)


def _fake_resample(input1, input2, kernel_size, op):
    if kernel_size < 1:
        raise ValueError("Resample2d: kernel_size must be >= 1")
    refuse(input2.dtype == input1.dtype, op, ": input2 has dtype ", input2.dtype, ", expected ", input1.dtype)
    refuse(input1.dtype in (torch.float32, torch.bfloat16), op, ": float32 tensors expected (bfloat16 is widened to float32), got ",
           input1.dtype)
    refuse(input1.dim() == 4 and input2.dim() == 4, op, ": tensors must be 4-D")
    refuse(input2.shape[1] == 2, op, ": input2 (flow) must have 2 channels, got ", input2.shape[1])
    refuse(input1.shape[0] == input2.shape[0], op, ": input1 ", tuple(input1.shape), " does not match the flow ", tuple(input2.shape))


def _resample2d_fake(input1, input2, kernel_size, bilinear):
    _fake_resample(input1, input2, kernel_size, "fn2::resample2d")
    return input1.new_empty((input2.shape[0], input1.shape[1], input2.shape[2], input2.shape[3]))


def _resample2d_backward_fake(input1, input2, grad_output, kernel_size, bilinear):
    _fake_resample(input1, input2, kernel_size, "fn2::resample2d_backward")
    return input1.new_empty(input1.shape), input2.new_empty(input2.shape)


def _resample2d_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.kernel_size, ctx.bilinear = inputs[2], inputs[3]


def _resample2d_grad(ctx, grad_output):
    input1, input2 = ctx.saved_tensors
    grad_input1, grad_input2 = _resample2d_backward_op(input1, input2, grad_output, ctx.kernel_size, ctx.bilinear)
    return grad_input1, grad_input2, None, None


_resample2d_op = fn2_ops.define("resample2d", "(Tensor input1, Tensor input2, int kernel_size, bool bilinear) -> Tensor",
                                _resample2d, _resample2d_fake, _resample2d_grad, _resample2d_setup)
# (backward_alloc reads torch.are_deterministic_algorithms_enabled() when the operator runs: the fixed-point path under compile too)
_resample2d_backward_op = fn2_ops.define(
    "resample2d_backward", "(Tensor input1, Tensor input2, Tensor grad_output, int kernel_size, bool bilinear) -> (Tensor, Tensor)",
    resample2d_cuda.backward_alloc, _resample2d_backward_fake)


# The fused warp rows.  Element types as the C++ nodes: x and flow of the same 16-bit type and (WarpDiffNormCat) no gradient for x ->
# the native 16-bit kernels, whose backward recomputes warp and norm; a 16-bit x that needs a gradient, or mixed types -> widened
# around the float32 kernels, each result rounded once.  The widened backward reads the float32 output BEFORE its rounding, so the
# forward operators return it next to the rounded one (numel 0 where nothing was widened): functional, and the eager node's bits.
def _warp_types(x, flow, x_needs_grad, cat):
    """(native16, widen) of WarpDiffNormCat (``cat``) / WarpDiffNorm."""
    same = x.dtype == flow.dtype
    if cat:
        native16 = same and x.dtype in _LOWP and not x_needs_grad
        return native16, not native16 and (x.dtype in _LOWP or not same)
    return same and x.dtype in _LOWP, not same


def _fake_warp(x, flow, op):
    refuse(x.dtype in _WARP_DTYPES, op, ": float32, float16 or bfloat16 tensors expected, got ", x.dtype)
    refuse(flow.dtype in _WARP_DTYPES, op, ": float32, float16 or bfloat16 tensors expected, got ", flow.dtype)
    refuse(x.dim() == 4 and flow.dim() == 4, op, ": tensors must be 4-D")
    refuse(x.shape[1] % 2 == 0 and x.shape[1] > 0, op, ": x must be 4-D with two images, got ", tuple(x.shape))
    refuse(flow.shape[0] == x.shape[0] and flow.shape[1] == 2 and flow.shape[2] == x.shape[2] and flow.shape[3] == x.shape[3], op,
           ": flow ", tuple(flow.shape), " does not match pair ", tuple(x.shape))


def _warp_diff_norm_cat(x_, flow_, div_flow, bilinear, x_needs_grad):
    _, widen = _warp_types(x_, flow_, x_needs_grad, True)
    x, flow = (x_.float() if widen else x_).contiguous(), (flow_.float() if widen else flow_).contiguous()
    b, c2, h, w = x.shape
    out = x.new_empty((b, c2 + c2 // 2 + 3, h, w))
    resample2d_cuda.warp_diff_norm_cat(x, flow, out, div_flow, bilinear)
    return (out.to(x_.dtype), out) if widen else (out, out.new_empty(0))


def _warp_diff_norm_cat_fake(x, flow, div_flow, bilinear, x_needs_grad):
    _fake_warp(x, flow, "fn2::warp_diff_norm_cat")
    _, widen = _warp_types(x, flow, x_needs_grad, True)
    shape = (x.shape[0], x.shape[1] + x.shape[1] // 2 + 3, x.shape[2], x.shape[3])
    return x.new_empty(shape), (x.new_empty(shape, dtype=torch.float32) if widen else x.new_empty(0))


def _warp_diff_norm_cat_backward(x_, flow_, out, wide, grad_out, div_flow, bilinear, need_x, need_flow):
    native16, widen = _warp_types(x_, flow_, need_x, True)
    x, flow = (x_.float() if widen else x_).contiguous(), (flow_.float() if widen else flow_).contiguous()
    out = wide if widen else (x.new_empty(0) if native16 else out)
    grad_x = torch.empty_like(x) if need_x else x.new_empty(0)
    grad_flow = torch.empty_like(flow)
    resample2d_cuda.warp_diff_norm_cat_backward(x, flow, out, grad_out.to(x.dtype).contiguous(), grad_x, grad_flow, div_flow, bilinear)
    return (grad_x.to(x_.dtype) if need_x else grad_x), grad_flow.to(flow_.dtype)


def _warp_diff_norm_cat_backward_fake(x, flow, out, wide, grad_out, div_flow, bilinear, need_x, need_flow):
    _fake_warp(x, flow, "fn2::warp_diff_norm_cat_backward")
    _, widen = _warp_types(x, flow, need_x, True)
    return (x.new_empty(x.shape) if need_x else x.new_empty(0, dtype=torch.float32 if widen else x.dtype)), flow.new_empty(flow.shape)


def _warp_diff_norm_cat_setup(ctx, inputs, output):
    x, flow, div_flow, bilinear, x_needs_grad = inputs
    if ctx.needs_input_grad[0] and not x_needs_grad:
        raise RuntimeError("fn2::warp_diff_norm_cat: x requires a gradient, so x_needs_grad must be True (it picks the kernels)")
    native16, _ = _warp_types(x, flow, x_needs_grad, True)
    ctx.save_for_backward(*((x, flow) if native16 else (x, flow) + tuple(output)))
    ctx.div_flow, ctx.bilinear = div_flow, bilinear


def _warp_diff_norm_cat_grad(ctx, grad_out, _grad_wide):
    need_x, need_flow = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (need_x or need_flow):
        return None, None, None, None, None
    x, flow = ctx.saved_tensors[:2]
    out, wide = ctx.saved_tensors[2:] if len(ctx.saved_tensors) > 2 else (x.new_empty(0), x.new_empty(0))
    grad_x, grad_flow = _warp_diff_norm_cat_backward_op(x, flow, out, wide, grad_out, ctx.div_flow, ctx.bilinear, need_x, need_flow)
    return (grad_x if need_x else None), (grad_flow if need_flow else None), None, None, None


_warp_diff_norm_cat_op = fn2_ops.define(
    "warp_diff_norm_cat", "(Tensor x, Tensor flow, float div_flow, bool bilinear, bool x_needs_grad) -> (Tensor, Tensor)",
    _warp_diff_norm_cat, _warp_diff_norm_cat_fake, _warp_diff_norm_cat_grad, _warp_diff_norm_cat_setup)
_warp_diff_norm_cat_backward_op = fn2_ops.define(
    "warp_diff_norm_cat_backward",
    "(Tensor x, Tensor flow, Tensor out, Tensor wide, Tensor grad_out, float div_flow, bool bilinear, bool need_x, bool need_flow)"
    " -> (Tensor, Tensor)", _warp_diff_norm_cat_backward, _warp_diff_norm_cat_backward_fake)


def _warp_diff_norm(x_, flow_, bilinear):
    _, widen = _warp_types(x_, flow_, False, False)
    x, flow = (x_.float() if widen else x_).contiguous(), (flow_.float() if widen else flow_).contiguous()
    norm = resample2d_cuda.warp_diff_norm(x, flow, bilinear)
    return (norm.to(x_.dtype), norm) if widen else (norm, norm.new_empty(0))


def _warp_diff_norm_fake(x, flow, bilinear):
    _fake_warp(x, flow, "fn2::warp_diff_norm")
    _, widen = _warp_types(x, flow, False, False)
    shape = (x.shape[0], 1, x.shape[2], x.shape[3])
    return x.new_empty(shape), (x.new_empty(shape, dtype=torch.float32) if widen else x.new_empty(0))


def _warp_diff_norm_backward(x_, flow_, norm, wide, grad_norm, bilinear):
    native16, widen = _warp_types(x_, flow_, False, False)
    x, flow = (x_.float() if widen else x_).contiguous(), (flow_.float() if widen else flow_).contiguous()
    norm = wide if widen else (x.new_empty(0) if native16 else norm)
    grad_flow = resample2d_cuda.warp_diff_norm_backward(x, flow, norm, grad_norm.to(x.dtype).contiguous(), bilinear)
    return grad_flow.to(flow_.dtype)


def _warp_diff_norm_backward_fake(x, flow, norm, wide, grad_norm, bilinear):
    _fake_warp(x, flow, "fn2::warp_diff_norm_backward")
    return flow.new_empty(flow.shape)


def _warp_diff_norm_setup(ctx, inputs, output):
    x, flow, bilinear = inputs
    native16, _ = _warp_types(x, flow, False, False)
    ctx.save_for_backward(*((x, flow) if native16 else (x, flow) + tuple(output)))
    ctx.bilinear = bilinear


def _warp_diff_norm_grad(ctx, grad_norm, _grad_wide):
    if not ctx.needs_input_grad[1]:
        return None, None, None
    x, flow = ctx.saved_tensors[:2]
    norm, wide = ctx.saved_tensors[2:] if len(ctx.saved_tensors) > 2 else (x.new_empty(0), x.new_empty(0))
    return None, _warp_diff_norm_backward_op(x, flow, norm, wide, grad_norm, ctx.bilinear), None


_warp_diff_norm_op = fn2_ops.define("warp_diff_norm", "(Tensor x, Tensor flow, bool bilinear) -> (Tensor, Tensor)",
                                    _warp_diff_norm, _warp_diff_norm_fake, _warp_diff_norm_grad, _warp_diff_norm_setup)
_warp_diff_norm_backward_op = fn2_ops.define(
    "warp_diff_norm_backward", "(Tensor x, Tensor flow, Tensor norm, Tensor wide, Tensor grad_norm, bool bilinear) -> Tensor",
    _warp_diff_norm_backward, _warp_diff_norm_backward_fake)


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
        if torch.compiler.is_compiling():   # Dynamo traces apply() through this method: the operator it can see
            return _resample2d_op(input1, input2, kernel_size, bilinear)
        # output: (B, C_img, H, W) with B, H, W from the flow (reference :16-18), allocated on the C++ side and fully written
        return resample2d_cuda.forward_alloc(input1, input2, kernel_size, bilinear)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input1, input2 = ctx.saved_tensors
        # grad_input1 is accumulated into by the kernel (fp32 atomics), so it starts at zero (reference resample2d.py:31): zeros and the
        # contiguous copy of grad_output are made on the C++ side.  (Folding the fill into the kernel was built and measured in round 5:
        # slower than this fill)
        backward_alloc = _resample2d_backward_op if torch.compiler.is_compiling() else resample2d_cuda.backward_alloc
        grad_input1, grad_input2 = backward_alloc(input1, input2, grad_output, ctx.kernel_size, ctx.bilinear)
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
        if torch.compiler.is_compiling():   # the operators widen, round and recompute as the lines below do
            out, wide = _warp_diff_norm_cat_op(x, flow, float(div_flow), bool(bilinear), ctx.needs_input_grad[0])
            ctx.save_for_backward(x, flow, out, wide)
            ctx.div_flow, ctx.bilinear = float(div_flow), bool(bilinear)
            return out
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
        need_x, need_flow = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_flow):
            return None, None, None, None
        if torch.compiler.is_compiling():
            x, flow, out, wide = ctx.saved_tensors
            grad_x, grad_flow = _warp_diff_norm_cat_backward_op(x, flow, out, wide, grad_out, ctx.div_flow, ctx.bilinear, need_x, need_flow)
            return (grad_x if need_x else None), (grad_flow if need_flow else None), None, None
        x, flow = ctx.saved_tensors[:2]
        out = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else x.new_empty(0)
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
        if torch.compiler.is_compiling():
            norm, wide = _warp_diff_norm_op(x, flow, bool(bilinear))
            ctx.save_for_backward(x, flow, norm, wide)
            ctx.bilinear = bool(bilinear)
            return norm
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
        if torch.compiler.is_compiling():
            x, flow, norm, wide = ctx.saved_tensors
            return None, _warp_diff_norm_backward_op(x, flow, norm, wide, grad_norm, ctx.bilinear), None
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
