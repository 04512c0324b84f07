// forward_warp_cuda.cpp -- pybind module `forward_warp_cuda`: ForwardWarp, forward flow splatting (include/flownet2_hip_splat.h)
// on the caller's current HIP stream.  Not one of the reference's modules: it links libflownet2_hip_splat.so only.
// forward / backward take caller-provided tensors and resize them in place; *_alloc return fresh tensors; apply is the
// differentiable op with its autograd node on the C++ side.  Everything is float32.  Under
// torch.use_deterministic_algorithms(True) (warn_only too) the forward takes the fixed-point entry point, its workspace from the
// caching allocator; the backward is a gather and the same in both modes.  No global state.
#include "binding_common.h"
#include "flownet2_hip_splat.h"

using namespace fn2b;

// the status text of libflownet2_hip_splat.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rcs(int rc, const char *op) { check_status(STATUS_SPLAT, rc, op); }

struct Geo {
    int B, C, H, W;
};

// binding_common.h's check_f32 behind a hint of this layer's own for half and bfloat16 tensors
static void check_f32_not16(const at::Tensor &t, const char *op, const char *name)
{
    const bool is16 = t.scalar_type() == at::kHalf || t.scalar_type() == at::kBFloat16;
    TORCH_CHECK(!is16, op, ": ", name, " must be float32, got ", t.scalar_type(),
                ": call .float() on it (a 16-bit accumulating output would round at every add)");
    check_f32(t, op, name);
}

// the arguments first, then where the tensors live: a wrong shape or dtype is reported as such on any device
static Geo check_inputs(const at::Tensor &input, const at::Tensor &flow, const char *op)
{
    TORCH_CHECK(input.defined() && flow.defined(), op, ": input or flow is undefined");
    TORCH_CHECK(input.dim() == 4 && flow.dim() == 4, op, ": input and flow must be 4-D (N, C, H, W); add the missing dimensions with [None]");
    TORCH_CHECK(input.size(1) >= 1, op, ": input has no channels");
    TORCH_CHECK(flow.size(1) == 2, op, ": flow has ", flow.size(1), " channels, expected 2 (x, y)");
    TORCH_CHECK(flow.size(0) == input.size(0) && flow.size(2) == input.size(2) && flow.size(3) == input.size(3), op, ": flow ", flow.sizes(),
                " must have the batch size, height and width of input ", input.sizes(),
                " (the output has the input's size; resize the flow first)");
    check_f32_not16(input, op, "input");
    check_f32_not16(flow, op, "flow");
    check_gpu(input, op, "input");
    check_gpu(flow, op, "flow");
    TORCH_CHECK(flow.device() == input.device(), op, ": flow is on ", flow.device(), ", expected ", input.device());
    return Geo{(int)input.size(0), (int)input.size(1), (int)input.size(2), (int)input.size(3)};
}

int forward_warp_forward_hip(at::Tensor &input, at::Tensor &flow, at::Tensor &output, int algo)
{
    const char *op = "forward_warp_cuda.forward";
    TORCH_CHECK(algo >= FN2S_AUTO && algo <= FN2S_TILED, op, ": algo ", algo, " is not 0 (auto), 1 (general) or 2 (tiled)");
    const Geo g = check_inputs(input, flow, op);
    check_same(input, output, op, "output");
    c10::DeviceGuard guard(input.device());
    at::Tensor a = input.contiguous(), f = flow.contiguous();
    output.resize_({g.B, g.C, g.H, g.W});   // cleared or fully written by the entry point, no fill_(0)
    TORCH_CHECK(output.is_contiguous(), op, ": output must be contiguous");
    if (deterministic()) {
        const size_t wsb = fn2s_forward_warp_forward_det_workspace_bytes(g.B, g.C, g.H, g.W);
        c10::DataPtr ws = det_workspace(wsb);
        check_rcs(fn2s_forward_warp_forward_det(a.data_ptr(), f.data_ptr(), output.data_ptr(), ws.get(), wsb, g.B, g.C, g.H, g.W,
                                                current_stream(input)), op);
    } else {
        check_rcs(fn2s_forward_warp_forward(a.data_ptr(), f.data_ptr(), output.data_ptr(), g.B, g.C, g.H, g.W, algo, current_stream(input)), op);
    }
    return 1;
}

// want_input / want_flow: which gradients to compute; the other tensor is left as it is
int forward_warp_backward_hip(at::Tensor &input, at::Tensor &flow, at::Tensor &gradOutput, at::Tensor &gradInput, at::Tensor &gradFlow,
                              bool want_input, bool want_flow)
{
    const char *op = "forward_warp_cuda.backward";
    TORCH_CHECK(want_input || want_flow, op, ": neither gradient is wanted");
    const Geo g = check_inputs(input, flow, op);
    check_same(input, gradOutput, op, "gradOutput");
    if (want_input) check_same(input, gradInput, op, "gradInput");
    if (want_flow) check_same(input, gradFlow, op, "gradFlow");
    TORCH_CHECK(gradOutput.dim() == 4 && gradOutput.sizes() == input.sizes(), op, ": gradOutput has shape ", gradOutput.sizes(), ", expected ",
                input.sizes());
    c10::DeviceGuard guard(input.device());
    at::Tensor a = input.contiguous(), f = flow.contiguous(), go = gradOutput.contiguous();
    if (want_input) gradInput.resize_({g.B, g.C, g.H, g.W});   // fully written, no fill_(0)
    if (want_flow) gradFlow.resize_({g.B, 2, g.H, g.W});
    TORCH_CHECK((!want_input || gradInput.is_contiguous()) && (!want_flow || gradFlow.is_contiguous()), op, ": gradients must be contiguous");
    check_rcs(fn2s_forward_warp_backward(a.data_ptr(), f.data_ptr(), go.data_ptr(), want_input ? gradInput.data_ptr() : nullptr,
                                         want_flow ? gradFlow.data_ptr() : nullptr, g.B, g.C, g.H, g.W, current_stream(input)), op);
    return 1;
}

at::Tensor forward_warp_forward_alloc(at::Tensor &input, at::Tensor &flow, int algo)
{
    TORCH_CHECK(algo >= FN2S_AUTO && algo <= FN2S_TILED, "forward_warp_cuda.forward_alloc: algo ", algo, " is not 0 (auto), 1 (general) or 2 (tiled)");
    check_inputs(input, flow, "forward_warp_cuda.forward_alloc");
    c10::DeviceGuard guard(input.device());
    at::Tensor output = unsized(input);
    forward_warp_forward_hip(input, flow, output, algo);
    return output;
}

// an undefined tensor (None in Python) for a gradient that is not wanted
std::vector<at::Tensor> forward_warp_backward_alloc(at::Tensor &input, at::Tensor &flow, at::Tensor &gradOutput, bool want_input, bool want_flow)
{
    TORCH_CHECK(want_input || want_flow, "forward_warp_cuda.backward_alloc: neither gradient is wanted");
    check_inputs(input, flow, "forward_warp_cuda.backward_alloc");
    c10::DeviceGuard guard(input.device());
    at::Tensor gi = want_input ? unsized(input) : at::Tensor(), gf = want_flow ? unsized(input) : at::Tensor();
    forward_warp_backward_hip(input, flow, gradOutput, gi, gf, want_input, want_flow);
    return {gi, gf};
}

// ---- autograd node on the C++ side, as convex_upsample_cuda.apply: no Python between `apply` and the launch
struct ForwardWarpOp : public torch::autograd::Function<ForwardWarpOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &input, const at::Tensor &flow)
    {
        ctx->save_for_backward({input, flow});
        at::Tensor a = input, f = flow;
        return forward_warp_forward_alloc(a, f, FN2S_AUTO);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "ForwardWarpFunction.backward");
        auto saved = ctx->get_saved_variables();
        at::Tensor a = saved[0], f = saved[1], go = grad_outputs[0];
        const bool wi = ctx->needs_input_grad(0), wf = ctx->needs_input_grad(1);
        if (!wi && !wf) return {at::Tensor(), at::Tensor()};
        auto g = forward_warp_backward_alloc(a, f, go, wi, wf);
        return {g[0], g[1]};
    }
};

at::Tensor forward_warp_apply(const at::Tensor &input, const at::Tensor &flow) { return ForwardWarpOp::apply(input, flow); }

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "ForwardWarp: forward flow splatting, gfx950 HIP kernels";
    m.def("apply", &forward_warp_apply, "ForwardWarpFunction.apply: differentiable in input and flow, autograd node on the C++ side",
          py::arg("input"), py::arg("flow"));
    m.def("forward_alloc", &forward_warp_forward_alloc, "forward returning a freshly allocated output", py::arg("input"), py::arg("flow"),
          py::arg("algo") = 0);
    m.def("backward_alloc", &forward_warp_backward_alloc, "backward returning freshly allocated gradients (input, flow); None for one not wanted",
          py::arg("input"), py::arg("flow"), py::arg("grad_output"), py::arg("want_input") = true, py::arg("want_flow") = true);
    m.def("forward", &forward_warp_forward_hip, "ForwardWarp forward (HIP, gfx950); output is resized in place", py::arg("input"),
          py::arg("flow"), py::arg("output"), py::arg("algo") = 0);
    m.def("backward", &forward_warp_backward_hip, "ForwardWarp backward (HIP, gfx950); the wanted gradients are resized in place",
          py::arg("input"), py::arg("flow"), py::arg("grad_output"), py::arg("grad_input"), py::arg("grad_flow"), py::arg("want_input") = true,
          py::arg("want_flow") = true);
    m.attr("AUTO") = (int)FN2S_AUTO;
    m.attr("GENERAL") = (int)FN2S_GENERAL;
    m.attr("TILED") = (int)FN2S_TILED;
}
