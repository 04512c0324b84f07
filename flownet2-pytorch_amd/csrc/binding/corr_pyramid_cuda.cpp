// corr_pyramid_cuda.cpp -- pybind module `corr_pyramid_cuda`: CorrPyramid, the build of RAFT's all-pairs correlation pyramid
// (CorrBlock.__init__; include/preview/flownet2_hip_pyramid.h) on the caller's current HIP stream.  An incubating module: it links
// libflownet2_hip_pyramid.so only.  *_alloc return fresh tensors; apply is the differentiable op with its autograd node on the C++
// side.  float32 only.  The backward is the fold kernel and two at::bmm.
#include "binding_common.h"
#include "preview/flownet2_hip_pyramid.h"

using namespace fn2b;

// the status text of libflownet2_hip_pyramid.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rcy(int rc, const char *op) { check_status(STATUS_PYRAMID, rc, op); }

struct Geo {
    int B, C, H, W, H2, W2, L;
};

// fmap1: B x C x H x W, fmap2: B x C x H2 x W2, contiguous float32 on one GPU
static Geo check_inputs(const at::Tensor &fmap1, const at::Tensor &fmap2, int64_t num_levels, const char *op)
{
    check_gpu(fmap1, op, "fmap1");
    check_same(fmap1, fmap2, op, "fmap2");
    // what the C ABI cannot see of a tensor is reported in its words: the dtype, the layout, a level count beyond an int
    if (fmap1.scalar_type() != at::kFloat) check_rcy(FN2_EDTYPE, op);
    TORCH_CHECK(fmap1.dim() == 4 && fmap2.dim() == 4 && fmap1.size(0) == fmap2.size(0) && fmap1.size(1) == fmap2.size(1), op, ": fmap1 ",
                fmap1.sizes(), " and fmap2 ", fmap2.sizes(), " must be [B, C, H, W] and [B, C, H2, W2]");
    if (!fmap1.is_contiguous() || !fmap2.is_contiguous() || num_levels < 1 || num_levels > FN2Y_MAX_LEVELS) check_rcy(FN2_EINVAL, op);
    for (const at::Tensor *t : {&fmap1, &fmap2})
        for (int d = 0; d < 4; ++d)
            if (t->size(d) > INT32_MAX) check_rcy(FN2_EUNSUPPORTED, op);
    return Geo{(int)fmap1.size(0), (int)fmap1.size(1), (int)fmap1.size(2), (int)fmap1.size(3), (int)fmap2.size(2), (int)fmap2.size(3),
               (int)num_levels};
}

std::vector<at::Tensor> corr_pyramid_forward_alloc(const at::Tensor &fmap1, const at::Tensor &fmap2, int64_t num_levels)
{
    const char *op = "corr_pyramid_cuda.forward";
    const Geo g = check_inputs(fmap1, fmap2, num_levels, op);
    c10::DeviceGuard guard(fmap1.device());
    std::vector<at::Tensor> levels;
    std::vector<void *> ptrs;
    const int64_t pixels = (int64_t)g.B * g.H * g.W;
    for (int l = 0; l < g.L; ++l) {
        levels.push_back(at::empty({pixels, 1, g.H2 >> l, g.W2 >> l}, fmap1.options()));   // fully written by the kernel, no fill_(0)
        ptrs.push_back(levels.back().data_ptr());
    }
    check_rcy(fn2y_corr_pyramid_forward(fmap1.data_ptr(), fmap2.data_ptr(), ptrs.data(), g.L, g.B, g.C, g.H, g.W, g.H2, g.W2,
                                        current_stream(fmap1)), op);
    return levels;
}

// (grad_fmap1, grad_fmap2) from the levels' gradients; an undefined entry is a missing gradient.  want1 / want2: which to compute
// (the other comes back undefined).
std::tuple<at::Tensor, at::Tensor> corr_pyramid_backward_alloc(const at::Tensor &fmap1, const at::Tensor &fmap2,
                                                               std::vector<c10::optional<at::Tensor>> grad_levels, bool want1, bool want2)
{
    const char *op = "corr_pyramid_cuda.backward";
    const Geo g = check_inputs(fmap1, fmap2, (int64_t)grad_levels.size(), op);
    const int64_t pixels = (int64_t)g.B * g.H * g.W;
    std::vector<at::Tensor> held;
    std::vector<const void *> ptrs;
    for (int l = 0; l < g.L; ++l) {
        if (!grad_levels[l].has_value() || !grad_levels[l]->defined()) {
            ptrs.push_back(nullptr);
            continue;
        }
        const at::Tensor &t = *grad_levels[l];
        check_same(fmap1, t, op, "a level's gradient");
        const bool four = t.dim() == 4 && t.size(1) == 1;
        TORCH_CHECK((four || t.dim() == 3) && t.size(0) == pixels && t.size(four ? 2 : 1) == (g.H2 >> l) && t.size(four ? 3 : 2) == (g.W2 >> l), op,
                    ": the gradient of level ", l, " has shape ", t.sizes(), ", expected [", pixels, ", 1, ", g.H2 >> l, ", ", g.W2 >> l, "]");
        held.push_back(t.contiguous());
        ptrs.push_back(held.back().data_ptr());
    }
    c10::DeviceGuard guard(fmap1.device());
    const int64_t M = (int64_t)g.H * g.W, N = (int64_t)g.H2 * g.W2;
    at::Tensor G = at::empty({g.B, M, N}, fmap1.options());   // fully written by the kernel
    check_rcy(fn2y_corr_pyramid_fold(ptrs.data(), g.L, G.data_ptr(), g.B, g.C, g.H, g.W, g.H2, g.W2, current_stream(fmap1)), op);
    at::Tensor g1, g2;
    if (want1) g1 = at::bmm(fmap2.view({g.B, g.C, N}), G.transpose(1, 2)).view(fmap1.sizes());
    if (want2) g2 = at::bmm(fmap1.view({g.B, g.C, M}), G).view(fmap2.sizes());
    return {g1, g2};
}

// ---- autograd node on the C++ side, as corr_sample_cuda.apply: no Python between `apply` and the launch
struct CorrPyramidOp : public torch::autograd::Function<CorrPyramidOp> {
    static variable_list forward(AutogradContext *ctx, const at::Tensor &fmap1, const at::Tensor &fmap2, int64_t num_levels)
    {
        ctx->save_for_backward({fmap1, fmap2});
        return corr_pyramid_forward_alloc(fmap1, fmap2, num_levels);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "CorrPyramidFunction.backward");
        auto saved = ctx->get_saved_variables();
        std::vector<c10::optional<at::Tensor>> grads;
        for (const at::Tensor &t : grad_outputs) grads.push_back(t.defined() ? c10::optional<at::Tensor>(t) : c10::nullopt);
        auto [g1, g2] = corr_pyramid_backward_alloc(saved[0], saved[1], grads, ctx->needs_input_grad(0), ctx->needs_input_grad(1));
        return {g1, g2, at::Tensor()};
    }
};

std::vector<at::Tensor> corr_pyramid_apply(const at::Tensor &fmap1, const at::Tensor &fmap2, int64_t num_levels)
{
    return CorrPyramidOp::apply(fmap1, fmap2, num_levels);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "CorrPyramid (incubating): the build of RAFT's all-pairs correlation pyramid in one fused MFMA kernel, gfx950 HIP kernels";
    m.def("apply", &corr_pyramid_apply, "CorrPyramidFunction.apply: differentiable in both feature maps, autograd node on the C++ side",
          py::arg("fmap1"), py::arg("fmap2"), py::arg("num_levels"));
    m.def("forward_alloc", &corr_pyramid_forward_alloc, "forward returning the freshly allocated levels");
    m.def("backward_alloc", &corr_pyramid_backward_alloc, "fold + two bmm: (grad_fmap1, grad_fmap2), undefined where not wanted",
          py::arg("fmap1"), py::arg("fmap2"), py::arg("grad_levels"), py::arg("want1") = true, py::arg("want2") = true);
}
