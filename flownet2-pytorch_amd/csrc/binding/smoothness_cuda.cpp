// smoothness_cuda.cpp -- pybind module `smoothness_cuda`: the edge-aware smoothness term (include/flownet2_hip_smooth.h) on the
// caller's current HIP stream.  Not one of the reference's modules: it links libflownet2_hip_smooth.so only.
// forward / backward take caller-provided tensors and resize them in place; *_alloc return fresh tensors; apply is the
// differentiable op with its autograd node on the C++ side.  The flow gets a gradient, the image does not: an image that requires
// one is refused at every door.  Everything is float32.  No global state.
#include "binding_common.h"
#include "flownet2_hip_smooth.h"

using namespace fn2b;

// the status text of libflownet2_hip_smooth.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rcm(int rc, const char *op) { check_status(STATUS_SMOOTH, rc, op); }

struct Geo {
    int N, F, C, H, W;
};

// the arguments first, then where the tensors live: a wrong shape, dtype or parameter is reported as such on any device
static Geo check_inputs(const at::Tensor &flow, const at::Tensor &image, int64_t order, int64_t edge, double alpha, double eps, const char *op)
{
    TORCH_CHECK(flow.defined() && image.defined(), op, ": flow or image is undefined");
    TORCH_CHECK(flow.dim() == 4 && image.dim() == 4, op, ": flow and image must be 4-D (N, channels, H, W); add the missing dimensions with [None]");
    TORCH_CHECK(flow.size(0) == image.size(0) && flow.size(2) == image.size(2) && flow.size(3) == image.size(3), op, ": image ", image.sizes(),
                " must have the batch, height and width of flow ", flow.sizes());
    TORCH_CHECK(flow.size(1) >= 1 && flow.size(1) <= FN2M_MAX_FLOW_CHANNELS, op, ": flow has ", flow.size(1), " channels, expected 1 to 4");
    TORCH_CHECK(image.size(1) == 1 || image.size(1) == 3, op, ": the image has ", image.size(1), " channels, expected 1 (grey) or 3 (RGB)");
    TORCH_CHECK(order == 1 || order == 2, op, ": order ", order, " is not 1 or 2");
    TORCH_CHECK(edge == FN2M_EDGE_EXPONENTIAL || edge == FN2M_EDGE_GAUSSIAN, op, ": edge_weighting ", edge, " is not 0 (exponential) or 1 (gaussian)");
    TORCH_CHECK(std::isfinite((float)alpha) && alpha >= 0, op, ": alpha ", alpha, " is not a finite float >= 0");
    TORCH_CHECK(std::isfinite((float)eps) && eps >= 0, op, ": eps ", eps, " is not a finite float >= 0");
    check_f32(flow, op, "flow");
    check_f32(image, op, "image");
    TORCH_CHECK(!image.requires_grad(), op, ": image requires a gradient, and this layer has none for the image (it is input data): pass image.detach()");
    check_gpu(flow, op, "flow");
    check_gpu(image, op, "image");
    TORCH_CHECK(image.device() == flow.device(), op, ": image is on ", image.device(), ", expected ", flow.device());
    return Geo{(int)flow.size(0), (int)flow.size(1), (int)image.size(1), (int)flow.size(2), (int)flow.size(3)};
}

int smoothness_forward_hip(at::Tensor &flow, at::Tensor &image, at::Tensor &output, int64_t order, int64_t edge, double alpha, double eps)
{
    const char *op = "smoothness_cuda.forward";
    const Geo g = check_inputs(flow, image, order, edge, alpha, eps, op);
    check_same(flow, output, op, "output");
    c10::DeviceGuard guard(flow.device());
    at::Tensor a = flow.contiguous(), b = image.contiguous();
    output.resize_({g.N, 2, g.H, g.W});   // fully written by the kernel, no fill_(0)
    TORCH_CHECK(output.is_contiguous(), op, ": output must be contiguous");
    check_rcm(fn2m_smoothness_forward(a.data_ptr(), b.data_ptr(), output.data_ptr(), g.N, g.F, g.C, g.H, g.W, (int)order, (int)edge, (float)alpha,
                                      (float)eps, current_stream(flow)), op);
    return 1;
}

int smoothness_backward_hip(at::Tensor &flow, at::Tensor &image, at::Tensor &gradOutput, at::Tensor &gradFlow, int64_t order, int64_t edge,
                            double alpha, double eps)
{
    const char *op = "smoothness_cuda.backward";
    const Geo g = check_inputs(flow, image, order, edge, alpha, eps, op);
    check_same(flow, gradOutput, op, "gradOutput");
    check_same(flow, gradFlow, op, "gradFlow");
    TORCH_CHECK(gradOutput.dim() == 4 && gradOutput.size(0) == g.N && gradOutput.size(1) == 2 && gradOutput.size(2) == g.H && gradOutput.size(3) == g.W,
                op, ": gradOutput has shape ", gradOutput.sizes(), ", expected [", g.N, ", 2, ", g.H, ", ", g.W, "]");
    c10::DeviceGuard guard(flow.device());
    at::Tensor a = flow.contiguous(), b = image.contiguous(), go = gradOutput.contiguous();
    gradFlow.resize_({g.N, g.F, g.H, g.W});   // fully written, no fill_(0)
    TORCH_CHECK(gradFlow.is_contiguous(), op, ": gradFlow must be contiguous");
    check_rcm(fn2m_smoothness_backward(a.data_ptr(), b.data_ptr(), go.data_ptr(), gradFlow.data_ptr(), g.N, g.F, g.C, g.H, g.W, (int)order, (int)edge,
                                       (float)alpha, (float)eps, current_stream(flow)), op);
    return 1;
}

at::Tensor smoothness_forward_alloc(at::Tensor &flow, at::Tensor &image, int64_t order, int64_t edge, double alpha, double eps)
{
    check_inputs(flow, image, order, edge, alpha, eps, "smoothness_cuda.forward_alloc");
    c10::DeviceGuard guard(flow.device());
    at::Tensor output = unsized(flow);
    smoothness_forward_hip(flow, image, output, order, edge, alpha, eps);
    return output;
}

at::Tensor smoothness_backward_alloc(at::Tensor &flow, at::Tensor &image, at::Tensor &gradOutput, int64_t order, int64_t edge, double alpha, double eps)
{
    check_inputs(flow, image, order, edge, alpha, eps, "smoothness_cuda.backward_alloc");
    c10::DeviceGuard guard(flow.device());
    at::Tensor grad = at::empty({0}, flow.options().requires_grad(false));
    smoothness_backward_hip(flow, image, gradOutput, grad, order, edge, alpha, eps);
    return grad;
}

// ---- autograd node on the C++ side, as census_cuda.apply: no Python between `apply` and the launch
struct SmoothnessOp : public torch::autograd::Function<SmoothnessOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &flow, const at::Tensor &image, int64_t order, int64_t edge, double alpha,
                              double eps)
    {
        ctx->save_for_backward({flow, image});
        ctx->saved_data["order"] = order;
        ctx->saved_data["edge"] = edge;
        ctx->saved_data["alpha"] = alpha;
        ctx->saved_data["eps"] = eps;
        at::Tensor a = flow, b = image;
        return smoothness_forward_alloc(a, b, order, edge, alpha, eps);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "SmoothnessFunction.backward");
        auto saved = ctx->get_saved_variables();
        at::Tensor a = saved[0], b = saved[1], go = grad_outputs[0];
        if (!ctx->needs_input_grad(0)) return {at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
        at::Tensor g = smoothness_backward_alloc(a, b, go, ctx->saved_data["order"].toInt(), ctx->saved_data["edge"].toInt(),
                                                 ctx->saved_data["alpha"].toDouble(), ctx->saved_data["eps"].toDouble());
        return {g, at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

at::Tensor smoothness_apply(const at::Tensor &flow, const at::Tensor &image, int64_t order, int64_t edge, double alpha, double eps)
{
    // in front of the node: inside it the inputs are detached views and no longer say whether they require a gradient
    check_inputs(flow, image, order, edge, alpha, eps, "smoothness_cuda.apply");
    return SmoothnessOp::apply(flow, image, order, edge, alpha, eps);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "Edge-aware smoothness of first or second order: the regulariser of unsupervised optical flow, gfx950 HIP kernels";
    m.def("apply", &smoothness_apply, "SmoothnessFunction.apply: differentiable in flow, autograd node on the C++ side", py::arg("flow"),
          py::arg("image"), py::arg("order") = 1, py::arg("edge_weighting") = 0, py::arg("alpha") = 150.0, py::arg("eps") = 0.001);
    m.def("forward_alloc", &smoothness_forward_alloc, "forward returning a freshly allocated N x 2 x H x W output", py::arg("flow"), py::arg("image"),
          py::arg("order") = 1, py::arg("edge_weighting") = 0, py::arg("alpha") = 150.0, py::arg("eps") = 0.001);
    m.def("backward_alloc", &smoothness_backward_alloc, "backward returning a freshly allocated gradient of flow", py::arg("flow"), py::arg("image"),
          py::arg("grad_output"), py::arg("order") = 1, py::arg("edge_weighting") = 0, py::arg("alpha") = 150.0, py::arg("eps") = 0.001);
    m.def("forward", &smoothness_forward_hip, "smoothness forward (HIP, gfx950); output is resized in place", py::arg("flow"), py::arg("image"),
          py::arg("output"), py::arg("order") = 1, py::arg("edge_weighting") = 0, py::arg("alpha") = 150.0, py::arg("eps") = 0.001);
    m.def("backward", &smoothness_backward_hip, "smoothness backward (HIP, gfx950); grad_flow is resized in place", py::arg("flow"),
          py::arg("image"), py::arg("grad_output"), py::arg("grad_flow"), py::arg("order") = 1, py::arg("edge_weighting") = 0,
          py::arg("alpha") = 150.0, py::arg("eps") = 0.001);
    m.attr("MAX_ORDER") = (int)FN2M_MAX_ORDER;
    m.attr("MAX_FLOW_CHANNELS") = (int)FN2M_MAX_FLOW_CHANNELS;
    m.attr("EDGE_EXPONENTIAL") = (int)FN2M_EDGE_EXPONENTIAL;
    m.attr("EDGE_GAUSSIAN") = (int)FN2M_EDGE_GAUSSIAN;
}
