// corr_sample1d_cuda.cpp -- pybind module `corr_sample1d_cuda`: CorrSample1d, the lookup of a prebuilt 1-D correlation pyramid
// (RAFT-Stereo's CorrBlock1D; include/staging/flownet2_hip_sample1d.h) on the caller's current HIP stream.  A staging module: it
// links libflownet2_hip_sample1d.so only.  *_alloc return fresh tensors; apply is the differentiable op with its autograd node on
// the C++ side.  float32 only; coords has no gradient.
#include <climits>

#include "binding_common.h"
#include "staging/flownet2_hip_sample1d.h"

using namespace fn2b;

// the status text of libflownet2_hip_sample1d.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rch(int rc, const char *op) { check_status(STATUS_SAMPLE1D, rc, op); }

struct Geo {
    int B, H, W, L;
    std::vector<int> W2;
};

// coords: B x 2 x H x W (channel 0 is read in place) or B x 1 x H x W; `levels`: how many the caller holds
static Geo check_coords(const at::Tensor &coords, size_t levels, int radius, const char *op)
{
    check_gpu(coords, op, "coords");
    check_f32(coords, op, "coords");
    TORCH_CHECK(levels >= 1 && levels <= (size_t)FN2H_MAX_LEVELS, op, ": the pyramid has ", levels, " levels, expected 1 .. ", FN2H_MAX_LEVELS);
    TORCH_CHECK(radius >= 0 && radius <= FN2H_MAX_RADIUS, op, ": radius ", radius, " outside 0 .. ", FN2H_MAX_RADIUS);
    TORCH_CHECK(coords.dim() == 4 && (coords.size(1) == 1 || coords.size(1) == 2), op, ": coords has shape ", coords.sizes(),
                ", expected [B, 2, H, W] (RAFT-Stereo's; channel 0 is read) or [B, 1, H, W]");
    // before any narrowing: the C ABI takes ints, and a wrapped size would pass its checks
    TORCH_CHECK(coords.size(0) <= INT_MAX && coords.size(2) <= INT_MAX && coords.size(3) <= INT_MAX, op, ": coords has shape ", coords.sizes(),
                ", a dimension of 2^31 or more is not supported: split the batch or the image");
    return Geo{(int)coords.size(0), (int)coords.size(2), (int)coords.size(3), (int)levels, {}};
}

static int level_width(int64_t w, const char *op)
{
    TORCH_CHECK(w <= INT_MAX, op, ": a pyramid level is ", w, " cells wide, 2^31 or more is not supported");
    return (int)w;
}

// pyramid: L tensors (B H W, 1, 1, W2_l) or (B H W, W2_l)
static Geo check_inputs(const std::vector<at::Tensor> &pyramid, const at::Tensor &coords, int radius, const char *op)
{
    Geo g = check_coords(coords, pyramid.size(), radius, op);
    const int64_t pixels = coords.size(0) * coords.size(2) * coords.size(3);
    for (const at::Tensor &lvl : pyramid) {
        check_gpu(lvl, op, "a pyramid level");
        TORCH_CHECK(lvl.device() == coords.device(), op, ": a pyramid level is on ", lvl.device(), ", expected ", coords.device());
        TORCH_CHECK(lvl.scalar_type() == at::kFloat, op, ": float32 tensors expected, got ", lvl.scalar_type(),
                    " (RAFT-Stereo builds its correlation volume in float: use .float())");
        const bool four = lvl.dim() == 4 && lvl.size(1) == 1 && lvl.size(2) == 1;
        TORCH_CHECK((four || lvl.dim() == 2) && lvl.size(0) == pixels, op, ": a pyramid level has shape ", lvl.sizes(), ", expected [", pixels,
                    ", 1, 1, W2] or [", pixels, ", W2] for coords ", coords.sizes());
        g.W2.push_back(level_width(lvl.size(four ? 3 : 1), op));
    }
    return g;
}

at::Tensor corr_sample1d_forward_alloc(std::vector<at::Tensor> pyramid, at::Tensor &coords, int radius)
{
    const char *op = "corr_sample1d_cuda.forward";
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
    at::Tensor output = at::empty({g.B, g.L * D, g.H, g.W}, coords.options());   // fully written by the kernel, no fill_(0)
    const long long cbs = (long long)c.size(1) * g.H * g.W;                      // (stride(0) of the contiguous tensor, also where B <= 1)
    check_rch(fn2h_corr_sample1d_forward(ptrs.data(), g.W2.data(), g.L, c.data_ptr(), cbs, output.data_ptr(), g.B, g.H, g.W, radius,
                                         current_stream(coords)), op);
    return output;
}

// The gradients of the levels.  The backward reads no level, so it takes their shapes, not the tensors: level l is
// (B H W, 1, 1, widths[l]) where dims[l] == 4 and (B H W, widths[l]) where dims[l] == 2, float32 on coords' device.
std::vector<at::Tensor> corr_sample1d_backward_alloc(at::Tensor &coords, at::Tensor &gradOutput, std::vector<int64_t> widths,
                                                     std::vector<int64_t> dims, int radius)
{
    const char *op = "corr_sample1d_cuda.backward";
    Geo g = check_coords(coords, widths.size(), radius, op);
    TORCH_CHECK(dims.size() == widths.size(), op, ": ", widths.size(), " widths but ", dims.size(), " dims");
    check_same(coords, gradOutput, op, "gradOutput");
    const int D = 2 * radius + 1;
    TORCH_CHECK(gradOutput.dim() == 4 && gradOutput.size(0) == g.B && gradOutput.size(1) == g.L * D && gradOutput.size(2) == g.H &&
                    gradOutput.size(3) == g.W,
                op, ": gradOutput has shape ", gradOutput.sizes(), ", expected [", g.B, ", ", g.L * D, ", ", g.H, ", ", g.W, "]");
    c10::DeviceGuard guard(coords.device());
    at::Tensor c = coords.contiguous(), go = gradOutput.contiguous();
    const int64_t pixels = coords.size(0) * coords.size(2) * coords.size(3);
    std::vector<at::Tensor> grads;
    std::vector<void *> ptrs;
    for (size_t l = 0; l < widths.size(); ++l) {
        TORCH_CHECK(dims[l] == 2 || dims[l] == 4, op, ": level ", l, " has ", dims[l], " dimensions, expected 2 ([P, W2]) or 4 ([P, 1, 1, W2])");
        TORCH_CHECK(widths[l] >= 1, op, ": level ", l, " is ", widths[l], " cells wide, expected at least 1");
        g.W2.push_back(level_width(widths[l], op));
        grads.push_back(dims[l] == 4 ? at::empty({pixels, 1, 1, widths[l]}, coords.options())   // fully written by the kernel: no zeros
                                     : at::empty({pixels, widths[l]}, coords.options()));
        ptrs.push_back(grads.back().data_ptr());
    }
    const long long cbs = (long long)c.size(1) * g.H * g.W;
    check_rch(fn2h_corr_sample1d_backward(g.W2.data(), g.L, c.data_ptr(), cbs, go.data_ptr(), ptrs.data(), g.B, g.H, g.W, radius,
                                          current_stream(coords)), op);
    return grads;
}

// ---- autograd node on the C++ side, as corr_sample_cuda.apply: no Python between `apply` and the launch.  It saves coords and
// the levels' shapes, not the levels: the backward reads none of them, and a pyramid is hundreds of megabytes.
struct CorrSample1dOp : public torch::autograd::Function<CorrSample1dOp> {
    static at::Tensor forward(AutogradContext *ctx, at::TensorList pyramid, const at::Tensor &coords, int64_t radius)
    {
        at::Tensor c = coords;
        at::Tensor out = corr_sample1d_forward_alloc(pyramid.vec(), c, (int)radius);   // (checks the shapes read below)
        std::vector<int64_t> widths, dims;
        for (const at::Tensor &t : pyramid) {
            widths.push_back(t.size(-1));
            dims.push_back(t.dim());
        }
        ctx->save_for_backward({coords});
        ctx->saved_data["widths"] = widths;
        ctx->saved_data["dims"] = dims;
        ctx->saved_data["radius"] = radius;
        return out;
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "CorrSample1dFunction.backward");
        at::Tensor c = ctx->get_saved_variables()[0], go = grad_outputs[0];
        variable_list grads = corr_sample1d_backward_alloc(c, go, ctx->saved_data["widths"].toIntVector(), ctx->saved_data["dims"].toIntVector(),
                                                           (int)ctx->saved_data["radius"].toInt());
        grads.push_back(at::Tensor());   // coords
        grads.push_back(at::Tensor());   // radius
        return grads;
    }
};

at::Tensor corr_sample1d_apply(std::vector<at::Tensor> pyramid, const at::Tensor &coords, int64_t radius)
{
    // a silent None for coords would train wrongly: RAFT-Stereo detaches coords in every iteration, and so must the caller
    TORCH_CHECK(!(coords.defined() && coords.requires_grad() && at::GradMode::is_enabled()), "corr_sample1d_cuda.apply",
                ": coords requires grad, but this layer has no gradient for coords (as RAFT-Stereo's sampler): pass coords.detach()");
    return CorrSample1dOp::apply(at::TensorList(pyramid), coords, radius);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "CorrSample1d (staging): lookup of a prebuilt 1-D correlation pyramid, RAFT-Stereo's CorrBlock1D, gfx950 HIP kernels";
    m.def("apply", &corr_sample1d_apply, "CorrSample1dFunction.apply: differentiable in the pyramid levels, autograd node on the C++ side",
          py::arg("pyramid"), py::arg("coords"), py::arg("radius"));
    m.def("forward_alloc", &corr_sample1d_forward_alloc, "forward returning a freshly allocated output");
    m.def("backward_alloc", &corr_sample1d_backward_alloc, "backward returning freshly allocated gradients of the levels, from their widths and dims", py::arg("coords"),
          py::arg("grad_output"), py::arg("widths"), py::arg("dims"), py::arg("radius"));
}
