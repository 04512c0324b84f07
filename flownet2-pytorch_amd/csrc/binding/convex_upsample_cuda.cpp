// convex_upsample_cuda.cpp -- pybind module `convex_upsample_cuda`: ConvexUpsample, the convex flow upsampling of RAFT and its
// descendants (include/flownet2_hip_upsample.h) on the caller's current HIP stream.  Not one of the reference's modules: it
// links libflownet2_hip_upsample.so only.  forward / backward take caller-provided tensors and resize them in place; *_alloc
// return fresh tensors; apply is the differentiable op with its autograd node on the C++ side.  flow, the output and their
// gradients are float32; mask (and its gradient) float32, float16 or bfloat16.  The backward's workspace is allocated here.
#include "binding_common.h"
#include "flownet2_hip_upsample.h"

using namespace fn2b;

// the status text of libflownet2_hip_upsample.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rcu(int rc, const char *op) { check_status(STATUS_UPSAMPLE, rc, op); }

struct Geo {
    int B, C, H, W, dtype;
};

// the arguments first, then where the tensors live: a wrong factor or shape is reported as such on any device
static Geo check_inputs(const at::Tensor &flow, const at::Tensor &mask, int factor, const char *op)
{
    TORCH_CHECK(flow.defined() && mask.defined(), op, ": flow or mask is undefined");
    TORCH_CHECK(factor == 2 || factor == 4 || factor == 8, op, ": factor ", factor, " is not 2, 4 or 8");
    TORCH_CHECK(flow.dim() == 4 && mask.dim() == 4, op, ": flow and mask must be 4-D (N, C, H, W)");
    TORCH_CHECK(flow.size(1) >= 1 && flow.size(1) <= FN2U_MAX_CHANNELS, op, ": flow has ", flow.size(1), " channels, 1 .. ", FN2U_MAX_CHANNELS,
                " are supported");
    TORCH_CHECK(mask.size(1) == 9 * factor * factor, op, ": mask has ", mask.size(1), " channels, expected 9 * factor^2 = ", 9 * factor * factor);
    TORCH_CHECK(mask.size(0) == flow.size(0) && mask.size(2) == flow.size(2) && mask.size(3) == flow.size(3), op, ": mask ", mask.sizes(),
                " must have the batch size, height and width of flow ", flow.sizes());
    TORCH_CHECK(flow.scalar_type() == at::kFloat, op, ": flow must be float32, got ", flow.scalar_type(),
                " (RAFT upsamples its flow in float under autocast: use .float())");
    TORCH_CHECK(mask.scalar_type() == at::kFloat || mask.scalar_type() == at::kHalf || mask.scalar_type() == at::kBFloat16, op,
                ": mask must be float32, float16 or bfloat16, got ", mask.scalar_type());
    check_gpu(flow, op, "flow");
    check_gpu(mask, op, "mask");
    TORCH_CHECK(flow.device() == mask.device(), op, ": mask is on ", mask.device(), ", expected ", flow.device());
    return Geo{(int)flow.size(0), (int)flow.size(1), (int)flow.size(2), (int)flow.size(3), dtype_of(mask, op)};
}

int convex_upsample_forward_hip(at::Tensor &flow, at::Tensor &mask, at::Tensor &output, int factor, double scale)
{
    const char *op = "convex_upsample_cuda.forward";
    const Geo g = check_inputs(flow, mask, factor, op);
    check_same(flow, output, op, "output");
    c10::DeviceGuard guard(flow.device());
    at::Tensor a = flow.contiguous(), m = mask.contiguous();
    output.resize_({g.B, g.C, (int64_t)factor * g.H, (int64_t)factor * g.W});   // fully written by the kernel, no fill_(0)
    TORCH_CHECK(output.is_contiguous(), op, ": output must be contiguous");
    check_rcu(fn2u_convex_upsample_forward(a.data_ptr(), m.data_ptr(), output.data_ptr(), g.dtype, g.B, g.C, g.H, g.W, factor, (float)scale,
                                           current_stream(flow)), op);
    return 1;
}

int convex_upsample_backward_hip(at::Tensor &flow, at::Tensor &mask, at::Tensor &gradOutput, at::Tensor &gradFlow, at::Tensor &gradMask,
                                 int factor, double scale)
{
    const char *op = "convex_upsample_cuda.backward";
    const Geo g = check_inputs(flow, mask, factor, op);
    check_same(flow, gradOutput, op, "gradOutput");
    check_same(flow, gradFlow, op, "gradFlow");
    check_same(mask, gradMask, op, "gradMask");
    TORCH_CHECK(gradOutput.dim() == 4 && gradOutput.size(0) == g.B && gradOutput.size(1) == g.C && gradOutput.size(2) == (int64_t)factor * g.H &&
                    gradOutput.size(3) == (int64_t)factor * g.W,
                op, ": gradOutput has shape ", gradOutput.sizes(), ", expected [", g.B, ", ", g.C, ", ", factor * g.H, ", ", factor * g.W, "]");
    c10::DeviceGuard guard(flow.device());
    at::Tensor a = flow.contiguous(), m = mask.contiguous(), go = gradOutput.contiguous();
    gradFlow.resize_({g.B, g.C, g.H, g.W});     // both fully written, no fill_(0)
    gradMask.resize_({g.B, 9 * factor * factor, g.H, g.W});
    TORCH_CHECK(gradFlow.is_contiguous() && gradMask.is_contiguous(), op, ": gradients must be contiguous");
    // the T planes of the header (9 C planes per item); the caching allocator keeps it alive for the stream's work
    const size_t bytes = fn2u_convex_upsample_backward_workspace_bytes(g.B, g.C, g.H, g.W);
    at::Tensor ws = at::empty({(int64_t)(bytes / sizeof(float))}, flow.options());
    check_rcu(fn2u_convex_upsample_backward(a.data_ptr(), m.data_ptr(), go.data_ptr(), gradFlow.data_ptr(), gradMask.data_ptr(),
                                            g.B == 0 ? nullptr : ws.data_ptr(), g.dtype, g.B, g.C, g.H, g.W, factor, (float)scale,
                                            current_stream(flow)), op);
    return 1;
}

at::Tensor convex_upsample_forward_alloc(at::Tensor &flow, at::Tensor &mask, int factor, double scale)
{
    check_inputs(flow, mask, factor, "convex_upsample_cuda.forward_alloc");
    c10::DeviceGuard guard(flow.device());
    at::Tensor output = unsized(flow);
    convex_upsample_forward_hip(flow, mask, output, factor, scale);
    return output;
}

std::vector<at::Tensor> convex_upsample_backward_alloc(at::Tensor &flow, at::Tensor &mask, at::Tensor &gradOutput, int factor, double scale)
{
    check_inputs(flow, mask, factor, "convex_upsample_cuda.backward_alloc");
    c10::DeviceGuard guard(flow.device());
    at::Tensor gf = unsized(flow), gm = unsized(mask);
    convex_upsample_backward_hip(flow, mask, gradOutput, gf, gm, factor, scale);
    return {gf, gm};
}

// ---- autograd node on the C++ side, as corr_lookup_cuda.apply: no Python between `apply` and the launch
struct ConvexUpsampleOp : public torch::autograd::Function<ConvexUpsampleOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &flow, const at::Tensor &mask, int64_t factor, double scale)
    {
        ctx->save_for_backward({flow, mask});
        ctx->saved_data["factor"] = factor;
        ctx->saved_data["scale"] = scale;
        at::Tensor a = flow, m = mask;
        return convex_upsample_forward_alloc(a, m, (int)factor, scale);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "ConvexUpsampleFunction.backward");
        auto saved = ctx->get_saved_variables();
        at::Tensor a = saved[0], m = saved[1], go = grad_outputs[0];
        auto g = convex_upsample_backward_alloc(a, m, go, (int)ctx->saved_data["factor"].toInt(), ctx->saved_data["scale"].toDouble());
        return {g[0], g[1], at::Tensor(), at::Tensor()};
    }
};

at::Tensor convex_upsample_apply(const at::Tensor &flow, const at::Tensor &mask, int64_t factor, double scale)
{
    return ConvexUpsampleOp::apply(flow, mask, factor, scale);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "ConvexUpsample: RAFT's convex flow upsampling, gfx950 HIP kernels";
    m.def("apply", &convex_upsample_apply, "ConvexUpsampleFunction.apply: differentiable in flow and mask, autograd node on the C++ side",
          py::arg("flow"), py::arg("mask"), py::arg("factor"), py::arg("scale"));
    m.def("forward_alloc", &convex_upsample_forward_alloc, "forward returning a freshly allocated output");
    m.def("backward_alloc", &convex_upsample_backward_alloc, "backward returning freshly allocated gradients (flow, mask)");
    m.def("forward", &convex_upsample_forward_hip, "ConvexUpsample forward (HIP, gfx950); output is resized in place");
    m.def("backward", &convex_upsample_backward_hip, "ConvexUpsample backward (HIP, gfx950); the gradients are resized in place");
}
