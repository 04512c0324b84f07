// resample2d_cuda.cpp -- pybind module `resample2d_cuda` (drop-in for the reference's module,
// resample2d_cuda.cc:6-31).  float32, as in the reference (resample2d_kernel.cu:221-230); forward / backward also take bfloat16
// tensors (mixed-precision training) by widening them to float32 around the float32 kernels -- see widen_bf16 below.  The fused warp
// rows (warp_diff_norm_cat, warp_diff_norm and their autograd nodes) take half and bfloat16 tensors natively (fn2_warp_diff_norm*_16:
// the float32 arithmetic, every result rounded once); only a pair that itself needs a gradient is widened around the float32 node.
#include "binding_common.h"

using namespace fn2b;

// The float32 tensors the kernels expect: float32 passes through, bfloat16 is widened (exact) once; anything else is refused with
// the reference's message.  The caller rounds each result to bfloat16 once (copy_ into the bfloat16 tensor).
static bool widen_bf16(const at::Tensor &t, const char *op)
{
    const bool bf = t.scalar_type() == at::kBFloat16;
    TORCH_CHECK(t.scalar_type() == at::kFloat || bf, op, ": float32 tensors expected (bfloat16 is widened to float32), got ",
                t.scalar_type());
    return bf;
}

// torch.use_deterministic_algorithms(True), warn_only included: the backward passes that scatter grad_input1 take the fixed-point entry
// points (fn2_*_backward_det), whose results do not depend on the order of the additions; the workspace comes from the caching allocator
// (deterministic() and det_workspace() of binding_common.h)

// half / bfloat16: the element types the 16-bit entry points of the fused warp rows take
static bool is_lowp(const at::Tensor &t) { return t.scalar_type() == at::kHalf || t.scalar_type() == at::kBFloat16; }
static void check_warp_dtype(const at::Tensor &t, const char *op)
{
    TORCH_CHECK(t.scalar_type() == at::kFloat || is_lowp(t), op, ": float32, float16 or bfloat16 tensors expected, got ", t.scalar_type());
}

static void strides4(const at::Tensor &t, int64_t s[4])
{
    for (int i = 0; i < 4; ++i) s[i] = t.stride(i);
}

// resample2d_cuda_forward (resample2d_cuda.cc:6-13).  `output` is allocated (zero-filled) by the
// Python wrapper with shape (B_flow, C_img, H_flow, W_flow) (resample2d.py:16-18).
int resample2d_forward_hip(at::Tensor &input1, at::Tensor &input2, at::Tensor &output, int kernel_size, bool bilinear)
{
    const char *op = "resample2d_cuda.forward";
    check_gpu(input1, op, "input1");
    check_same(input1, input2, op, "input2");
    check_same(input1, output, op, "output");
    const bool bf = widen_bf16(input1, op);
    TORCH_CHECK(input1.dim() == 4 && input2.dim() == 4 && output.dim() == 4, op, ": tensors must be 4-D");
    TORCH_CHECK(input2.size(1) == 2, op, ": input2 (flow) must have 2 channels, got ", input2.size(1));
    const int B = output.size(0), C = output.size(1), H = output.size(2), W = output.size(3);
    TORCH_CHECK(input2.size(0) == B && input2.size(2) == H && input2.size(3) == W, op, ": flow ", input2.sizes(),
                " does not match output ", output.sizes());
    TORCH_CHECK(input1.size(0) == B && input1.size(1) == C, op, ": input1 ", input1.sizes(), " does not match output ",
                output.sizes());
    TORCH_CHECK(output.is_contiguous(), op, ": output must be contiguous");
    c10::DeviceGuard guard(input1.device());
    at::Tensor img = bf ? input1.to(at::kFloat) : input1;
    at::Tensor flow = bf ? input2.to(at::kFloat).contiguous() : input2.contiguous();
    at::Tensor out = bf ? at::empty(output.sizes(), output.options().dtype(at::kFloat)) : output;
    int64_t is[4];
    strides4(img, is); // honoured by the kernel, like the reference's DIM3_INDEX
    check_rc(fn2_resample2d_forward(img.data_ptr<float>(), is, flow.data_ptr<float>(), out.data_ptr<float>(), B,
                                    C, (int)img.size(2), (int)img.size(3), H, W, kernel_size, bilinear ? 1 : 0,
                                    current_stream(input1)), op);
    if (bf) output.copy_(out);
    return 1;
}

// resample2d_cuda_backward (resample2d_cuda.cc:15-24).  gradInput1 arrives zero-filled and is
// accumulated into; gradInput2 is overwritten (resample2d.py:31-36).
int resample2d_backward_hip(at::Tensor &input1, at::Tensor &input2, at::Tensor &gradOutput, at::Tensor &gradInput1,
                            at::Tensor &gradInput2, int kernel_size, bool bilinear)
{
    const char *op = "resample2d_cuda.backward";
    check_gpu(input1, op, "input1");
    check_same(input1, input2, op, "input2");
    check_same(input1, gradOutput, op, "gradOutput");
    check_same(input1, gradInput1, op, "gradInput1");
    check_same(input1, gradInput2, op, "gradInput2");
    const bool bf = widen_bf16(input1, op);
    TORCH_CHECK(input1.dim() == 4 && input2.dim() == 4 && gradOutput.dim() == 4, op, ": tensors must be 4-D");
    const int B = gradOutput.size(0), C = gradOutput.size(1), H = gradOutput.size(2), W = gradOutput.size(3);
    TORCH_CHECK(input2.size(0) == B && input2.size(1) == 2 && input2.size(2) == H && input2.size(3) == W, op,
                ": flow ", input2.sizes(), " does not match gradOutput ", gradOutput.sizes());
    TORCH_CHECK(input1.size(0) == B && input1.size(1) == C, op, ": input1 ", input1.sizes(),
                " does not match gradOutput ", gradOutput.sizes());
    TORCH_CHECK(gradInput1.sizes() == input1.sizes() && gradInput1.is_contiguous(), op,
                ": gradInput1 must be contiguous and shaped like input1");
    TORCH_CHECK(gradInput2.sizes() == input2.sizes() && gradInput2.is_contiguous(), op,
                ": gradInput2 must be contiguous and shaped like input2");
    c10::DeviceGuard guard(input1.device());
    // bfloat16: gradInput1 is accumulated in float32 (never with bfloat16 atomics, which round at every addition) and rounded once
    at::Tensor img = bf ? input1.to(at::kFloat) : input1;
    at::Tensor flow = bf ? input2.to(at::kFloat).contiguous() : input2.contiguous();
    at::Tensor go = bf ? gradOutput.to(at::kFloat).contiguous() : gradOutput.contiguous();
    at::Tensor g1 = bf ? gradInput1.to(at::kFloat) : gradInput1;
    at::Tensor g2 = bf ? at::empty(gradInput2.sizes(), gradInput2.options().dtype(at::kFloat)) : gradInput2;
    int64_t is[4];
    strides4(img, is);
    const int Hi = (int)img.size(2), Wi = (int)img.size(3);
    if (deterministic()) {   // torch.use_deterministic_algorithms(True) (warn_only too): gradInput1 summed in fixed point
        const size_t wsb = fn2_resample2d_backward_det_workspace_bytes(B, C, Hi, Wi, H, W, kernel_size);
        c10::DataPtr ws = det_workspace(wsb);
        check_rc(fn2_resample2d_backward_det(img.data_ptr<float>(), is, flow.data_ptr<float>(), go.data_ptr<float>(), g1.data_ptr<float>(),
                                             g2.data_ptr<float>(), B, C, Hi, Wi, H, W, kernel_size, bilinear ? 1 : 0, ws.get(), wsb,
                                             current_stream(input1)), op);
    } else {
        check_rc(fn2_resample2d_backward(img.data_ptr<float>(), is, flow.data_ptr<float>(), go.data_ptr<float>(),
                                         g1.data_ptr<float>(), g2.data_ptr<float>(), B, C,
                                         Hi, Wi, H, W, kernel_size, bilinear ? 1 : 0,
                                         current_stream(input1)), op);
    }
    if (bf) {
        gradInput1.copy_(g1);
        gradInput2.copy_(g2);
    }
    return 1;
}

// N2, not in the reference module: cat(pair, warp(pair[:, C:], flow), flow / div_flow,
// channelnorm(pair[:, :C] - warped)) in one pass (models.py:133-138).
int warp_diff_norm_cat_hip(at::Tensor &pair, at::Tensor &flow, at::Tensor &output, double div_flow, bool bilinear)
{
    const char *op = "resample2d_cuda.warp_diff_norm_cat";
    check_gpu(pair, op, "pair");
    check_same(pair, flow, op, "flow");
    check_same(pair, output, op, "output");
    check_warp_dtype(pair, op);
    TORCH_CHECK(pair.dim() == 4 && flow.dim() == 4 && output.dim() == 4, op, ": tensors must be 4-D");
    TORCH_CHECK(pair.size(1) % 2 == 0 && pair.size(1) > 0, op, ": pair must hold two images (even channel count), got ",
                pair.sizes());
    const int B = pair.size(0), C = pair.size(1) / 2, H = pair.size(2), W = pair.size(3);
    TORCH_CHECK(flow.size(0) == B && flow.size(1) == 2 && flow.size(2) == H && flow.size(3) == W, op, ": flow ",
                flow.sizes(), " does not match pair ", pair.sizes());
    TORCH_CHECK(output.size(0) == B && output.size(1) == 3 * C + 3 && output.size(2) == H && output.size(3) == W &&
                    output.is_contiguous(),
                op, ": output must be contiguous [", B, ", ", 3 * C + 3, ", ", H, ", ", W, "], got ", output.sizes());
    c10::DeviceGuard guard(pair.device());
    at::Tensor p = pair.contiguous(), f = flow.contiguous();
    if (is_lowp(pair)) {
        check_rc(fn2_warp_diff_norm_cat_16(p.data_ptr(), f.data_ptr(), output.data_ptr(), dtype_of(pair, op), (float)div_flow, B, C, H, W,
                                           bilinear ? 1 : 0, current_stream(pair)), op);
        return 1;
    }
    check_rc(fn2_warp_diff_norm_cat(p.data_ptr<float>(), f.data_ptr<float>(), output.data_ptr<float>(), (float)div_flow,
                                    B, C, H, W, bilinear ? 1 : 0, current_stream(pair)), op);
    return 1;
}

// Backward of warp_diff_norm_cat (fn2_warp_diff_norm_cat_backward).  gradPair: an empty tensor (numel 0) = not wanted.
int warp_diff_norm_cat_backward_hip(at::Tensor &pair, at::Tensor &flow, at::Tensor &output, at::Tensor &gradOutput,
                                    at::Tensor &gradPair, at::Tensor &gradFlow, double div_flow, bool bilinear)
{
    const char *op = "resample2d_cuda.warp_diff_norm_cat_backward";
    check_gpu(pair, op, "pair");
    check_same(pair, flow, op, "flow");
    check_same(pair, gradOutput, op, "gradOutput");
    check_same(pair, gradFlow, op, "gradFlow");
    check_warp_dtype(pair, op);
    const bool lowp = is_lowp(pair);   // half / bfloat16: flow gradient only, warp and norm recomputed; `output` is not read
    if (!lowp) check_same(pair, output, op, "output");
    TORCH_CHECK(pair.dim() == 4 && flow.dim() == 4 && gradOutput.dim() == 4 && (lowp || output.dim() == 4), op, ": tensors must be 4-D");
    TORCH_CHECK(pair.size(1) % 2 == 0 && pair.size(1) > 0, op, ": pair must hold two images, got ", pair.sizes());
    const int B = pair.size(0), C = pair.size(1) / 2, H = pair.size(2), W = pair.size(3);
    TORCH_CHECK(flow.size(0) == B && flow.size(1) == 2 && flow.size(2) == H && flow.size(3) == W, op, ": flow ", flow.sizes(),
                " does not match pair ", pair.sizes());
    TORCH_CHECK((lowp || output.sizes() == gradOutput.sizes()) && gradOutput.size(0) == B && gradOutput.size(1) == 3 * C + 3 &&
                    gradOutput.size(2) == H && gradOutput.size(3) == W, op, ": output / gradOutput must be [", B, ", ", 3 * C + 3, ", ", H, ", ", W, "]");
    TORCH_CHECK(pair.is_contiguous() && flow.is_contiguous() && (lowp || output.is_contiguous()), op, ": pair, flow and output must be contiguous");
    TORCH_CHECK(gradFlow.sizes() == flow.sizes() && gradFlow.is_contiguous(), op, ": gradFlow must be contiguous and shaped like flow");
    const bool want_pair = gradPair.defined() && gradPair.numel() > 0;
    if (want_pair) {
        check_same(pair, gradPair, op, "gradPair");
        TORCH_CHECK(gradPair.sizes() == pair.sizes() && gradPair.is_contiguous(), op, ": gradPair must be contiguous and shaped like pair");
    }
    c10::DeviceGuard guard(pair.device());
    at::Tensor go = gradOutput.contiguous();
    if (lowp) {
        TORCH_CHECK(!want_pair, op, ": the 16-bit backward gives the flow gradient only (the pair's gradient is a float32 scatter: widen the "
                                    "tensors, or use warp_diff_norm_cat_apply, which does)");
        check_rc(fn2_warp_diff_norm_cat_backward_16(pair.data_ptr(), flow.data_ptr(), go.data_ptr(), gradFlow.data_ptr(), dtype_of(pair, op),
                                                    (float)div_flow, B, C, H, W, bilinear ? 1 : 0, current_stream(pair)), op);
        return 1;
    }
    if (want_pair && deterministic()) {   // the second image's gradient is scattered: fixed-point sums under the deterministic flag
        const size_t wsb = fn2_warp_diff_norm_cat_backward_det_workspace_bytes(B, C, H, W);
        c10::DataPtr ws = det_workspace(wsb);
        check_rc(fn2_warp_diff_norm_cat_backward_det(pair.data_ptr<float>(), flow.data_ptr<float>(), output.data_ptr<float>(),
                                                     go.data_ptr<float>(), gradPair.data_ptr<float>(), gradFlow.data_ptr<float>(),
                                                     (float)div_flow, B, C, H, W, bilinear ? 1 : 0, ws.get(), wsb, current_stream(pair)),
                 op);
        return 1;
    }
    check_rc(fn2_warp_diff_norm_cat_backward(pair.data_ptr<float>(), flow.data_ptr<float>(), output.data_ptr<float>(), go.data_ptr<float>(),
                                             want_pair ? gradPair.data_ptr<float>() : nullptr, gradFlow.data_ptr<float>(), (float)div_flow,
                                             B, C, H, W, bilinear ? 1 : 0, current_stream(pair)), op);
    return 1;
}

// models.py:157-161 / :170-174: ||pair[:, :C] - warp(pair[:, C:], flow)||_2 (fn2_warp_diff_norm) and its flow gradient
at::Tensor warp_diff_norm_hip(at::Tensor &pair, at::Tensor &flow, bool bilinear)
{
    const char *op = "resample2d_cuda.warp_diff_norm";
    check_gpu(pair, op, "pair");
    check_same(pair, flow, op, "flow");
    check_warp_dtype(pair, op);
    TORCH_CHECK(pair.dim() == 4 && flow.dim() == 4 && pair.size(1) % 2 == 0 && pair.size(1) > 0, op, ": pair must be 4-D with two images");
    const int B = pair.size(0), C = pair.size(1) / 2, H = pair.size(2), W = pair.size(3);
    TORCH_CHECK(flow.size(0) == B && flow.size(1) == 2 && flow.size(2) == H && flow.size(3) == W, op, ": flow ", flow.sizes(),
                " does not match pair ", pair.sizes());
    c10::DeviceGuard guard(pair.device());
    at::Tensor p = pair.contiguous(), f = flow.contiguous();
    at::Tensor out = at::empty({B, 1, H, W}, pair.options());
    if (is_lowp(pair)) {
        check_rc(fn2_warp_diff_norm_16(p.data_ptr(), f.data_ptr(), out.data_ptr(), dtype_of(pair, op), B, C, H, W, bilinear ? 1 : 0,
                                       current_stream(pair)), op);
        return out;
    }
    check_rc(fn2_warp_diff_norm(p.data_ptr<float>(), f.data_ptr<float>(), out.data_ptr<float>(), B, C, H, W, bilinear ? 1 : 0,
                                current_stream(pair)), op);
    return out;
}

at::Tensor warp_diff_norm_backward_hip(at::Tensor &pair, at::Tensor &flow, at::Tensor &norm, at::Tensor &gradNorm, bool bilinear)
{
    const char *op = "resample2d_cuda.warp_diff_norm_backward";
    check_gpu(pair, op, "pair");
    check_same(pair, flow, op, "flow");
    check_same(pair, gradNorm, op, "gradNorm");
    check_warp_dtype(pair, op);
    const bool lowp = is_lowp(pair);   // half / bfloat16: the norm is recomputed, `norm` is not read (an empty tensor will do)
    if (!lowp) check_same(pair, norm, op, "norm");
    TORCH_CHECK(pair.dim() == 4 && flow.dim() == 4 && pair.size(1) % 2 == 0 && pair.size(1) > 0, op, ": pair must be 4-D with two images");
    const int B = pair.size(0), C = pair.size(1) / 2, H = pair.size(2), W = pair.size(3);
    TORCH_CHECK(flow.size(0) == B && flow.size(1) == 2 && flow.size(2) == H && flow.size(3) == W, op, ": flow ", flow.sizes(),
                " does not match pair ", pair.sizes());
    TORCH_CHECK(gradNorm.dim() == 4 && gradNorm.size(0) == B && gradNorm.size(1) == 1 && gradNorm.size(2) == H && gradNorm.size(3) == W, op,
                ": norm / gradNorm must be [", B, ", 1, ", H, ", ", W, "]");
    TORCH_CHECK(lowp || norm.sizes() == gradNorm.sizes(), op, ": norm / gradNorm must be [", B, ", 1, ", H, ", ", W, "]");
    TORCH_CHECK(pair.is_contiguous() && flow.is_contiguous() && (lowp || norm.is_contiguous()), op, ": pair, flow and norm must be contiguous");
    c10::DeviceGuard guard(pair.device());
    at::Tensor gn = gradNorm.contiguous();
    at::Tensor gflow = at::empty(flow.sizes(), flow.options());
    if (lowp) {
        check_rc(fn2_warp_diff_norm_backward_16(pair.data_ptr(), flow.data_ptr(), gn.data_ptr(), gflow.data_ptr(), dtype_of(pair, op), B, C, H, W,
                                                bilinear ? 1 : 0, current_stream(pair)), op);
        return gflow;
    }
    check_rc(fn2_warp_diff_norm_backward(pair.data_ptr<float>(), flow.data_ptr<float>(), norm.data_ptr<float>(), gn.data_ptr<float>(),
                                         gflow.data_ptr<float>(), B, C, H, W, bilinear ? 1 : 0, current_stream(pair)), op);
    return gflow;
}

// forward / backward with their outputs allocated here (the wrappers of this repository; the reference's signatures stay above)
at::Tensor resample2d_forward_alloc(at::Tensor &input1, at::Tensor &input2, int kernel_size, bool bilinear)
{
    const char *op = "resample2d_cuda.forward_alloc";
    check_gpu(input1, op, "input1");
    check_same(input1, input2, op, "input2");
    TORCH_CHECK(input1.dim() == 4 && input2.dim() == 4, op, ": tensors must be 4-D");
    c10::DeviceGuard guard(input1.device());
    at::Tensor output = at::empty({input2.size(0), input1.size(1), input2.size(2), input2.size(3)}, input1.options());   // (resample2d.py:16-18)
    resample2d_forward_hip(input1, input2, output, kernel_size, bilinear);
    return output;
}

std::vector<at::Tensor> resample2d_backward_alloc(at::Tensor &input1, at::Tensor &input2, at::Tensor &gradOutput, int kernel_size, bool bilinear)
{
    const char *op = "resample2d_cuda.backward_alloc";
    check_gpu(input1, op, "input1");
    check_same(input1, input2, op, "input2");
    c10::DeviceGuard guard(input1.device());
    at::Tensor g1 = at::zeros(input1.sizes(), input1.options());        // accumulated into: starts at zero (resample2d.py:31)
    at::Tensor g2 = at::empty(input2.sizes(), input2.options());        // fully written
    resample2d_backward_hip(input1, input2, gradOutput, g1, g2, kernel_size, bilinear);
    return {g1, g2};
}

// ---- autograd Functions on the C++ side: no Python between `apply` and the launch, no GIL in the backward.
// Same semantics as the Python Functions of networks/resample2d_package/resample2d.py.
struct Resample2dOp : public torch::autograd::Function<Resample2dOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &input1, const at::Tensor &input2, int64_t kernel_size, bool bilinear)
    {
        TORCH_CHECK(input2.is_contiguous(), "Resample2dFunction: flow must be contiguous (reference resample2d.py:10)");
        ctx->save_for_backward({input1, input2});
        ctx->saved_data["k"] = kernel_size;
        ctx->saved_data["b"] = bilinear;
        at::Tensor a = input1, f = input2;
        return resample2d_forward_alloc(a, f, (int)kernel_size, bilinear);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "Resample2dFunction.backward");
        auto saved = ctx->get_saved_variables();
        at::Tensor a = saved[0], f = saved[1], go = grad_outputs[0];
        auto g = resample2d_backward_alloc(a, f, go, (int)ctx->saved_data["k"].toInt(), ctx->saved_data["b"].toBool());
        return {g[0], g[1], at::Tensor(), at::Tensor()};
    }
};

at::Tensor resample2d_apply(const at::Tensor &input1, const at::Tensor &input2, int64_t kernel_size, bool bilinear)
{
    return Resample2dOp::apply(input1, input2, kernel_size, bilinear);
}

// models.py:133-138 as one differentiable op (fn2_warp_diff_norm_cat / fn2_warp_diff_norm_cat_backward).
// Element types: float32 as ever.  x and flow of the SAME 16-bit type (half, bfloat16) and no gradient wanted for x: the native 16-bit
// entry points, forward and backward; the backward recomputes the warp and the norm, so the node does not save its output.  A 16-bit x
// that needs a gradient itself, or mixed types (float32 x with a bfloat16 flow under autocast): widened around the float32 kernels,
// every result rounded once to its input's type (the output to x's).
struct WarpDiffNormCatOp : public torch::autograd::Function<WarpDiffNormCatOp> {
    // x_needs_grad: x.requires_grad() under the caller's grad mode (grad mode is off in here)
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &x_, const at::Tensor &flow_, double div_flow, bool bilinear, bool x_needs_grad)
    {
        const char *op = "WarpDiffNormCat";
        check_gpu(x_, op, "x");
        check_gpu(flow_, op, "flow");
        TORCH_CHECK(x_.device() == flow_.device(), op, ": flow is on ", flow_.device(), ", expected ", x_.device());
        check_warp_dtype(x_, op);
        check_warp_dtype(flow_, op);
        TORCH_CHECK(x_.dim() == 4 && x_.size(1) % 2 == 0 && x_.size(1) > 0, op, ": x must be 4-D with two images, got ", x_.sizes());
        c10::DeviceGuard guard(x_.device());
        const bool same = x_.scalar_type() == flow_.scalar_type();
        const bool native16 = same && is_lowp(x_) && !x_needs_grad;
        const bool widen = !native16 && (is_lowp(x_) || !same);
        at::Tensor x = (widen ? x_.to(at::kFloat) : x_).contiguous(), flow = (widen ? flow_.to(at::kFloat) : flow_).contiguous();
        const int64_t c2 = x.size(1);
        at::Tensor out = at::empty({x.size(0), c2 + c2 / 2 + 3, x.size(2), x.size(3)}, x.options());
        warp_diff_norm_cat_hip(x, flow, out, div_flow, bilinear);
        if (native16) ctx->save_for_backward({x, flow});
        else ctx->save_for_backward({x, flow, out});
        ctx->saved_data["d"] = div_flow;
        ctx->saved_data["b"] = bilinear;
        ctx->saved_data["tx"] = (int64_t)x_.scalar_type();
        ctx->saved_data["tf"] = (int64_t)flow_.scalar_type();
        return widen ? out.to(x_.scalar_type()) : out;
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "WarpDiffNormCatFunction.backward");
        const bool need_x = ctx->needs_input_grad(0), need_flow = ctx->needs_input_grad(1);
        if (!(need_x || need_flow)) return {at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
        auto saved = ctx->get_saved_variables();
        at::Tensor x = saved[0], flow = saved[1], out = saved.size() > 2 ? saved[2] : at::Tensor();
        c10::DeviceGuard guard(x.device());
        at::Tensor go = grad_outputs[0].to(x.scalar_type()).contiguous();   // (widened path: the 16-bit gradient widened, exact)
        at::Tensor gx = need_x ? at::empty_like(x) : unsized(x);
        at::Tensor gflow = at::empty_like(flow);
        if (!out.defined()) out = unsized(x);
        warp_diff_norm_cat_backward_hip(x, flow, out, go, gx, gflow, ctx->saved_data["d"].toDouble(), ctx->saved_data["b"].toBool());
        const auto tx = (at::ScalarType)ctx->saved_data["tx"].toInt(), tf = (at::ScalarType)ctx->saved_data["tf"].toInt();
        return {need_x ? gx.to(tx) : at::Tensor(), need_flow ? gflow.to(tf) : at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

at::Tensor warp_diff_norm_cat_apply(const at::Tensor &x, const at::Tensor &flow, double div_flow, bool bilinear)
{
    return WarpDiffNormCatOp::apply(x, flow, div_flow, bilinear, x.requires_grad() && at::GradMode::is_enabled());
}

// models.py:157-161 / :170-174 as one differentiable op (flow gradient only; the caller composes the unfused layers when the pair
// itself needs a gradient).  Element types as WarpDiffNormCatOp: same-type half / bfloat16 native (nothing but x and flow saved),
// mixed types widened.
struct WarpDiffNormOp : public torch::autograd::Function<WarpDiffNormOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &x_, const at::Tensor &flow_, bool bilinear)
    {
        const char *op = "WarpDiffNorm";
        check_gpu(x_, op, "x");
        check_gpu(flow_, op, "flow");
        check_warp_dtype(x_, op);
        check_warp_dtype(flow_, op);
        c10::DeviceGuard guard(x_.device());
        const bool same = x_.scalar_type() == flow_.scalar_type();
        const bool native16 = same && is_lowp(x_);
        const bool widen = !same;
        at::Tensor x = (widen ? x_.to(at::kFloat) : x_).contiguous(), flow = (widen ? flow_.to(at::kFloat) : flow_).contiguous();
        at::Tensor norm = warp_diff_norm_hip(x, flow, bilinear);
        if (native16) ctx->save_for_backward({x, flow});
        else ctx->save_for_backward({x, flow, norm});
        ctx->saved_data["b"] = bilinear;
        ctx->saved_data["tf"] = (int64_t)flow_.scalar_type();
        return widen ? norm.to(x_.scalar_type()) : norm;
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "WarpDiffNormFunction.backward");
        if (!ctx->needs_input_grad(1)) return {at::Tensor(), at::Tensor(), at::Tensor()};
        auto saved = ctx->get_saved_variables();
        at::Tensor x = saved[0], flow = saved[1], norm = saved.size() > 2 ? saved[2] : unsized(saved[0]);
        at::Tensor gn = grad_outputs[0].to(x.scalar_type());
        at::Tensor gflow = warp_diff_norm_backward_hip(x, flow, norm, gn, ctx->saved_data["b"].toBool());
        return {at::Tensor(), gflow.to((at::ScalarType)ctx->saved_data["tf"].toInt()), at::Tensor()};
    }
};

at::Tensor warp_diff_norm_apply(const at::Tensor &x, const at::Tensor &flow, bool bilinear)
{
    return WarpDiffNormOp::apply(x, flow, bilinear);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.def("apply", &resample2d_apply, "Resample2dFunction.apply: differentiable, autograd node on the C++ side", py::arg("input1"), py::arg("input2"),
          py::arg("kernel_size") = 1, py::arg("bilinear") = true);
    m.def("warp_diff_norm_cat_apply", &warp_diff_norm_cat_apply, "WarpDiffNormCatFunction.apply: differentiable, autograd node on the C++ side");
    m.def("warp_diff_norm_apply", &warp_diff_norm_apply, "WarpDiffNormFunction.apply: differentiable, autograd node on the C++ side");
    m.def("forward_alloc", &resample2d_forward_alloc, "forward returning a freshly allocated output");
    m.def("backward_alloc", &resample2d_backward_alloc, "backward returning freshly allocated gradients");
    m.doc() = "FlowNet2 Resample2d layer, gfx950 HIP kernels (drop-in for the reference resample2d_cuda)";
    m.def("forward", &resample2d_forward_hip, "Resample2D forward (HIP, gfx950)");
    m.def("backward", &resample2d_backward_hip, "Resample2D backward (HIP, gfx950)");
    m.def("warp_diff_norm_cat", &warp_diff_norm_cat_hip,
          "cat(pair, warp(second image, flow), flow / div_flow, ||first image - warped||) in one pass");
    m.def("warp_diff_norm_cat_backward", &warp_diff_norm_cat_backward_hip, "backward of warp_diff_norm_cat in one pass");
    m.def("warp_diff_norm", &warp_diff_norm_hip, "||first image - warp(second image, flow)|| in one pass (models.py:157-161)");
    m.def("warp_diff_norm_backward", &warp_diff_norm_backward_hip, "flow gradient of warp_diff_norm in one pass");
}
