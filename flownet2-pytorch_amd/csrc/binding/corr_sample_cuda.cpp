// corr_sample_cuda.cpp -- pybind module `corr_sample_cuda`: CorrSample, the lookup of a prebuilt all-pairs correlation pyramid
// (RAFT's CorrBlock; include/preview/flownet2_hip_sample.h) on the caller's current HIP stream.  A preview module: it links
// libflownet2_hip_sample.so only.  *_alloc return fresh tensors; apply is the differentiable op with its autograd node on the
// C++ side.  float32 only; coords has no gradient.
#include "binding_common.h"
#include "preview/flownet2_hip_sample.h"

using namespace fn2b;

// the status text of libflownet2_hip_sample.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rcp(int rc, const char *op) { check_status(STATUS_SAMPLE, rc, op); }

struct Geo {
    int B, H, W, L;
    std::vector<int> H2, W2;
};

// pyramid: L tensors (B H W, 1, H2_l, W2_l) or (B H W, H2_l, W2_l); coords: B x 2 x H x W
static Geo check_inputs(const std::vector<at::Tensor> &pyramid, const at::Tensor &coords, int radius, const char *op)
{
    check_gpu(coords, op, "coords");
    check_f32(coords, op, "coords");
    TORCH_CHECK(!pyramid.empty() && (int)pyramid.size() <= FN2P_MAX_LEVELS, op, ": the pyramid has ", pyramid.size(), " levels, expected 1 .. ",
                FN2P_MAX_LEVELS);
    TORCH_CHECK(radius >= 0 && radius <= FN2P_MAX_RADIUS, op, ": radius ", radius, " outside 0 .. ", FN2P_MAX_RADIUS);
    TORCH_CHECK(coords.dim() == 4 && coords.size(1) == 2, op, ": coords has shape ", coords.sizes(), ", expected [B, 2, H, W]");
    Geo g{(int)coords.size(0), (int)coords.size(2), (int)coords.size(3), (int)pyramid.size(), {}, {}};
    const int64_t pixels = coords.size(0) * coords.size(2) * coords.size(3);
    for (const at::Tensor &lvl : pyramid) {
        check_gpu(lvl, op, "a pyramid level");
        TORCH_CHECK(lvl.device() == coords.device(), op, ": a pyramid level is on ", lvl.device(), ", expected ", coords.device());
        TORCH_CHECK(lvl.scalar_type() == at::kFloat, op, ": float32 tensors expected, got ", lvl.scalar_type(),
                    " (RAFT builds its correlation volume in float: use .float())");
        const bool four = lvl.dim() == 4 && lvl.size(1) == 1;
        TORCH_CHECK((four || lvl.dim() == 3) && lvl.size(0) == pixels, op, ": a pyramid level has shape ", lvl.sizes(), ", expected [", pixels,
                    ", 1, H2, W2] for coords ", coords.sizes());
        g.H2.push_back((int)lvl.size(four ? 2 : 1));
        g.W2.push_back((int)lvl.size(four ? 3 : 2));
    }
    return g;
}

at::Tensor corr_sample_forward_alloc(std::vector<at::Tensor> pyramid, at::Tensor &coords, int radius)
{
    const char *op = "corr_sample_cuda.forward";
    const Geo g = check_inputs(pyramid, coords, radius, op);
    c10::DeviceGuard guard(coords.device());
    at::Tensor c = coords.contiguous();
    std::vector<at::Tensor> lv;
    std::vector<const void *> ptrs;
    for (const at::Tensor &t : pyramid) {
        lv.push_back(t.contiguous());
        ptrs.push_back(lv.back().data_ptr());
    }
    const int D = 2 * radius + 1;
    at::Tensor output = at::empty({g.B, g.L * D * D, g.H, g.W}, coords.options());   // fully written by the kernel, no fill_(0)
    check_rcp(fn2p_corr_sample_forward(ptrs.data(), g.H2.data(), g.W2.data(), g.L, c.data_ptr(), output.data_ptr(), g.B, g.H, g.W, radius,
                                       current_stream(coords)), op);
    return output;
}

// the gradients of the levels, in the levels' shapes; `pyramid` gives the shapes only
std::vector<at::Tensor> corr_sample_backward_alloc(std::vector<at::Tensor> pyramid, at::Tensor &coords, at::Tensor &gradOutput, int radius)
{
    const char *op = "corr_sample_cuda.backward";
    const Geo g = check_inputs(pyramid, coords, radius, op);
    check_same(coords, gradOutput, op, "gradOutput");
    const int D = 2 * radius + 1;
    TORCH_CHECK(gradOutput.dim() == 4 && gradOutput.size(0) == g.B && gradOutput.size(1) == g.L * D * D && gradOutput.size(2) == g.H &&
                    gradOutput.size(3) == g.W,
                op, ": gradOutput has shape ", gradOutput.sizes(), ", expected [", g.B, ", ", g.L * D * D, ", ", g.H, ", ", g.W, "]");
    c10::DeviceGuard guard(coords.device());
    at::Tensor c = coords.contiguous(), go = gradOutput.contiguous();
    std::vector<at::Tensor> grads;
    std::vector<void *> ptrs;
    for (const at::Tensor &t : pyramid) {
        grads.push_back(at::empty(t.sizes(), t.options()));   // fully written by the kernel: no zeros
        ptrs.push_back(grads.back().data_ptr());
    }
    check_rcp(fn2p_corr_sample_backward(g.H2.data(), g.W2.data(), g.L, c.data_ptr(), go.data_ptr(), ptrs.data(), g.B, g.H, g.W, radius,
                                        current_stream(coords)), op);
    return grads;
}

// ---- autograd node on the C++ side, as corr_lookup_cuda.apply: no Python between `apply` and the launch
struct CorrSampleOp : public torch::autograd::Function<CorrSampleOp> {
    static at::Tensor forward(AutogradContext *ctx, at::TensorList pyramid, const at::Tensor &coords, int64_t radius)
    {
        std::vector<at::Tensor> saved(pyramid.begin(), pyramid.end());   // (for their shapes; autograd holds them anyway)
        saved.push_back(coords);
        ctx->save_for_backward(saved);
        ctx->saved_data["radius"] = radius;
        at::Tensor c = coords;
        return corr_sample_forward_alloc(pyramid.vec(), c, (int)radius);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "CorrSampleFunction.backward");
        auto saved = ctx->get_saved_variables();
        at::Tensor c = saved.back(), go = grad_outputs[0];
        saved.pop_back();
        variable_list grads = corr_sample_backward_alloc(saved, c, go, (int)ctx->saved_data["radius"].toInt());
        grads.push_back(at::Tensor());   // coords
        grads.push_back(at::Tensor());   // radius
        return grads;
    }
};

at::Tensor corr_sample_apply(std::vector<at::Tensor> pyramid, const at::Tensor &coords, int64_t radius)
{
    // a silent None for coords would train wrongly: RAFT detaches coords in every iteration, and so must the caller
    TORCH_CHECK(!(coords.defined() && coords.requires_grad() && at::GradMode::is_enabled()), "corr_sample_cuda.apply",
                ": coords requires grad, but this layer has no gradient for coords (as RAFT's alt_cuda_corr): pass coords.detach()");
    return CorrSampleOp::apply(at::TensorList(pyramid), coords, radius);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "CorrSample (preview): lookup of a prebuilt all-pairs correlation pyramid, RAFT's CorrBlock, gfx950 HIP kernels";
    m.def("apply", &corr_sample_apply, "CorrSampleFunction.apply: differentiable in the pyramid levels, autograd node on the C++ side",
          py::arg("pyramid"), py::arg("coords"), py::arg("radius"));
    m.def("forward_alloc", &corr_sample_forward_alloc, "forward returning a freshly allocated output");
    m.def("backward_alloc", &corr_sample_backward_alloc, "backward returning freshly allocated gradients of the levels");
}
