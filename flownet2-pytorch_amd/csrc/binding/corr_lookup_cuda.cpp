// corr_lookup_cuda.cpp -- pybind module `corr_lookup_cuda`: CorrLookup, the on-demand correlation lookup of RAFT and its
// descendants (include/flownet2_hip_lookup.h) on the caller's current HIP stream.  Not one of the reference's modules: it links
// libflownet2_hip_lookup.so only.  forward / backward take caller-provided tensors and resize them in place; *_alloc return fresh
// tensors; apply is the differentiable op with its autograd node on the C++ side.  float32 only; coords has no gradient.
#include "binding_common.h"
#include "flownet2_hip_lookup.h"

using namespace fn2b;

// the status text of libflownet2_hip_lookup.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rcl(int rc, const char *op) { check_status(STATUS_LOOKUP, rc, op); }

struct Geo {
    int B, C, H, W, H2, W2;
};

static Geo check_inputs(const at::Tensor &fmap1, const at::Tensor &fmap2, const at::Tensor &coords, const char *op)
{
    check_gpu(fmap1, op, "fmap1");
    check_same(fmap1, fmap2, op, "fmap2");
    check_same(fmap1, coords, op, "coords");
    TORCH_CHECK(fmap1.scalar_type() == at::kFloat, op, ": float32 tensors expected, got ", fmap1.scalar_type(),
                " (RAFT calls its lookup in float under autocast: use .float())");
    TORCH_CHECK(fmap1.dim() == 4 && fmap2.dim() == 4 && coords.dim() == 4, op, ": fmap1, fmap2 and coords must be 4-D (N, C, H, W)");
    TORCH_CHECK(fmap2.size(0) == fmap1.size(0) && fmap2.size(1) == fmap1.size(1), op, ": fmap2 ", fmap2.sizes(),
                " must have the batch and channel counts of fmap1 ", fmap1.sizes());
    TORCH_CHECK(coords.size(0) == fmap1.size(0) && coords.size(1) == 2 && coords.size(2) == fmap1.size(2) && coords.size(3) == fmap1.size(3),
                op, ": coords has shape ", coords.sizes(), ", expected [", fmap1.size(0), ", 2, ", fmap1.size(2), ", ", fmap1.size(3), "]");
    return Geo{(int)fmap1.size(0), (int)fmap1.size(1), (int)fmap1.size(2), (int)fmap1.size(3), (int)fmap2.size(2), (int)fmap2.size(3)};
}

int corr_lookup_forward_hip(at::Tensor &fmap1, at::Tensor &fmap2, at::Tensor &coords, at::Tensor &output, int radius, double scale)
{
    const char *op = "corr_lookup_cuda.forward";
    const Geo g = check_inputs(fmap1, fmap2, coords, op);
    check_same(fmap1, output, op, "output");
    TORCH_CHECK(radius >= 0 && radius <= FN2L_MAX_RADIUS, op, ": radius ", radius, " outside 0 .. ", FN2L_MAX_RADIUS);
    c10::DeviceGuard guard(fmap1.device());
    at::Tensor a = fmap1.contiguous(), b = fmap2.contiguous(), c = coords.contiguous();
    const int D = 2 * radius + 1;
    output.resize_({g.B, D * D, g.H, g.W});   // fully written by the kernel, no fill_(0)
    TORCH_CHECK(output.is_contiguous(), op, ": output must be contiguous");
    check_rcl(fn2l_corr_lookup_forward(a.data_ptr(), b.data_ptr(), c.data_ptr(), output.data_ptr(), FN2_F32, g.B, g.C, g.H, g.W, g.H2, g.W2,
                                       radius, (float)scale, FN2L_LOOKUP_AUTO, current_stream(fmap1)), op);
    return 1;
}

int corr_lookup_backward_hip(at::Tensor &fmap1, at::Tensor &fmap2, at::Tensor &coords, at::Tensor &gradOutput, at::Tensor &gradFmap1,
                             at::Tensor &gradFmap2, int radius, double scale)
{
    const char *op = "corr_lookup_cuda.backward";
    const Geo g = check_inputs(fmap1, fmap2, coords, op);
    check_same(fmap1, gradOutput, op, "gradOutput");
    check_same(fmap1, gradFmap1, op, "gradFmap1");
    check_same(fmap1, gradFmap2, op, "gradFmap2");
    TORCH_CHECK(radius >= 0 && radius <= FN2L_MAX_RADIUS, op, ": radius ", radius, " outside 0 .. ", FN2L_MAX_RADIUS);
    const int D = 2 * radius + 1;
    TORCH_CHECK(gradOutput.dim() == 4 && gradOutput.size(0) == g.B && gradOutput.size(1) == D * D && gradOutput.size(2) == g.H &&
                    gradOutput.size(3) == g.W,
                op, ": gradOutput has shape ", gradOutput.sizes(), ", expected [", g.B, ", ", D * D, ", ", g.H, ", ", g.W, "]");
    // grad_fmap2 is summed by float atomics in arrival order
    if (deterministic()) at::globalContext().alertNotDeterministic("corr_lookup_cuda.backward");
    c10::DeviceGuard guard(fmap1.device());
    at::Tensor a = fmap1.contiguous(), b = fmap2.contiguous(), c = coords.contiguous(), go = gradOutput.contiguous();
    gradFmap1.resize_({g.B, g.C, g.H, g.W});     // fully written, no fill_(0); grad_fmap2 is cleared by the library on the stream
    gradFmap2.resize_({g.B, g.C, g.H2, g.W2});
    TORCH_CHECK(gradFmap1.is_contiguous() && gradFmap2.is_contiguous(), op, ": gradients must be contiguous");
    check_rcl(fn2l_corr_lookup_backward(a.data_ptr(), b.data_ptr(), c.data_ptr(), go.data_ptr(), gradFmap1.data_ptr(), gradFmap2.data_ptr(),
                                        FN2_F32, g.B, g.C, g.H, g.W, g.H2, g.W2, radius, (float)scale, FN2L_LOOKUP_AUTO,
                                        current_stream(fmap1)), op);
    return 1;
}

at::Tensor corr_lookup_forward_alloc(at::Tensor &fmap1, at::Tensor &fmap2, at::Tensor &coords, int radius, double scale)
{
    check_gpu(fmap1, "corr_lookup_cuda.forward_alloc", "fmap1");
    c10::DeviceGuard guard(fmap1.device());
    at::Tensor output = unsized(fmap1);
    corr_lookup_forward_hip(fmap1, fmap2, coords, output, radius, scale);
    return output;
}

std::vector<at::Tensor> corr_lookup_backward_alloc(at::Tensor &fmap1, at::Tensor &fmap2, at::Tensor &coords, at::Tensor &gradOutput,
                                                   int radius, double scale)
{
    check_gpu(fmap1, "corr_lookup_cuda.backward_alloc", "fmap1");
    c10::DeviceGuard guard(fmap1.device());
    at::Tensor g1 = unsized(fmap1), g2 = unsized(fmap1);
    corr_lookup_backward_hip(fmap1, fmap2, coords, gradOutput, g1, g2, radius, scale);
    return {g1, g2};
}

// ---- autograd node on the C++ side, as correlation1d_cuda.apply: no Python between `apply` and the launch
struct CorrLookupOp : public torch::autograd::Function<CorrLookupOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &fmap1, const at::Tensor &fmap2, const at::Tensor &coords,
                              int64_t radius, double scale)
    {
        ctx->save_for_backward({fmap1, fmap2, coords});
        ctx->saved_data["radius"] = radius;
        ctx->saved_data["scale"] = scale;
        at::Tensor a = fmap1, b = fmap2, c = coords;
        return corr_lookup_forward_alloc(a, b, c, (int)radius, scale);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "CorrLookupFunction.backward");
        auto saved = ctx->get_saved_variables();
        at::Tensor a = saved[0], b = saved[1], c = saved[2], go = grad_outputs[0];
        auto g = corr_lookup_backward_alloc(a, b, c, go, (int)ctx->saved_data["radius"].toInt(), ctx->saved_data["scale"].toDouble());
        return {g[0], g[1], at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

at::Tensor corr_lookup_apply(const at::Tensor &fmap1, const at::Tensor &fmap2, const at::Tensor &coords, int64_t radius, double scale)
{
    // a silent None for coords would train wrongly: RAFT detaches coords in every iteration, and so must the caller
    TORCH_CHECK(!(coords.defined() && coords.requires_grad() && at::GradMode::is_enabled()), "corr_lookup_cuda.apply",
                ": coords requires grad, but this layer has no gradient for coords (as RAFT's alt_cuda_corr): pass coords.detach()");
    return CorrLookupOp::apply(fmap1, fmap2, coords, radius, scale);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "CorrLookup: RAFT's on-demand correlation lookup, gfx950 HIP kernels";
    m.def("apply", &corr_lookup_apply, "CorrLookupFunction.apply: differentiable in fmap1 and fmap2, autograd node on the C++ side",
          py::arg("fmap1"), py::arg("fmap2"), py::arg("coords"), py::arg("radius"), py::arg("scale"));
    m.def("forward_alloc", &corr_lookup_forward_alloc, "forward returning a freshly allocated output");
    m.def("backward_alloc", &corr_lookup_backward_alloc, "backward returning freshly allocated gradients");
    m.def("forward", &corr_lookup_forward_hip, "CorrLookup forward (HIP, gfx950); output is resized in place");
    m.def("backward", &corr_lookup_backward_hip, "CorrLookup backward (HIP, gfx950); the gradients are resized in place");
}
