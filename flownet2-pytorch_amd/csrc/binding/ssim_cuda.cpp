// ssim_cuda.cpp -- pybind module `ssim_cuda`: the structural-similarity distance (include/staging/flownet2_hip_ssim.h) on the
// caller's current HIP stream.  Not one of the reference's modules: it links libflownet2_hip_ssim.so only.
// forward / backward take caller-provided tensors and resize them in place; *_alloc return fresh tensors; apply is the
// differentiable op with its autograd node on the C++ side, which asks only for the gradients that are needed.  Everything is
// float32.  Inputs that are not contiguous (channels-last, a slice) are copied first, as census_cuda does.  No global state.
#include "binding_common.h"
#include "staging/flownet2_hip_ssim.h"

using namespace fn2b;

// the status text of libflownet2_hip_ssim.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rci(int rc, const char *op) { check_status(STATUS_SSIM, rc, op); }

struct Geo {
    int N, C, H, W;
};

// the arguments first, then where the tensors live: a wrong shape, dtype or parameter is reported as such on any device
static Geo check_inputs(const at::Tensor &im1, const at::Tensor &im2, int64_t md, double c1, double c2, int64_t border, const char *op)
{
    TORCH_CHECK(im1.defined() && im2.defined(), op, ": im1 or im2 is undefined");
    TORCH_CHECK(im1.dim() == 4 && im2.dim() == 4, op, ": im1 and im2 must be 4-D (N, C, H, W); add the missing dimensions with [None]");
    TORCH_CHECK(im1.sizes() == im2.sizes(), op, ": im2 ", im2.sizes(), " must have the shape of im1 ", im1.sizes());
    TORCH_CHECK(im1.size(1) >= 1 && im1.size(2) >= 1 && im1.size(3) >= 1, op, ": the images ", im1.sizes(), " have an empty channel, row or column dimension");
    TORCH_CHECK(md >= 1 && md <= FN2I_MAX_DISTANCE, op, ": max_distance ", md, " is not 1, 2 or 3");
    TORCH_CHECK(std::isfinite((float)c1) && (float)c1 > 0.f, op, ": c1 ", c1, " is not a finite float above 0");
    TORCH_CHECK(std::isfinite((float)c2) && (float)c2 > 0.f, op, ": c2 ", c2, " is not a finite float above 0");
    TORCH_CHECK(border == FN2I_BORDER_ZERO || border == FN2I_BORDER_REFLECT, op, ": border code ", border, " is not 0 (zero) or 1 (reflect)");
    TORCH_CHECK(border != FN2I_BORDER_REFLECT || (im1.size(2) > md && im1.size(3) > md), op, ": border reflect needs H and W above max_distance ", md,
                ", got ", im1.size(2), " x ", im1.size(3), ": use border zero or a smaller max_distance");
    check_f32(im1, op, "im1");
    check_f32(im2, op, "im2");
    check_gpu(im1, op, "im1");
    check_gpu(im2, op, "im2");
    TORCH_CHECK(im2.device() == im1.device(), op, ": im2 is on ", im2.device(), ", expected ", im1.device());
    return Geo{(int)im1.size(0), (int)im1.size(1), (int)im1.size(2), (int)im1.size(3)};
}

int ssim_forward_hip(at::Tensor &im1, at::Tensor &im2, at::Tensor &output, int64_t md, double c1, double c2, int64_t border)
{
    const char *op = "ssim_cuda.forward";
    const Geo g = check_inputs(im1, im2, md, c1, c2, border, op);
    check_same(im1, output, op, "output");
    c10::DeviceGuard guard(im1.device());
    at::Tensor a = im1.contiguous(), b = im2.contiguous();
    output.resize_({g.N, g.C, g.H, g.W});   // fully written by the kernel, no fill_(0)
    TORCH_CHECK(output.is_contiguous(), op, ": output must be contiguous");
    check_rci(fn2i_ssim_forward(a.data_ptr(), b.data_ptr(), output.data_ptr(), g.N, g.C, g.H, g.W, (int)md, (float)c1, (float)c2, (int)border,
                                current_stream(im1)), op);
    return 1;
}

// want1 / want2: which gradients to compute; the other tensor is left as it is
int ssim_backward_hip(at::Tensor &im1, at::Tensor &im2, at::Tensor &gradOutput, at::Tensor &grad1, at::Tensor &grad2, int64_t md, double c1,
                      double c2, int64_t border, bool want1, bool want2)
{
    const char *op = "ssim_cuda.backward";
    TORCH_CHECK(want1 || want2, op, ": neither gradient is wanted");
    const Geo g = check_inputs(im1, im2, md, c1, c2, border, op);
    check_same(im1, gradOutput, op, "gradOutput");
    if (want1) check_same(im1, grad1, op, "grad1");
    if (want2) check_same(im1, grad2, op, "grad2");
    TORCH_CHECK(gradOutput.sizes() == im1.sizes(), op, ": gradOutput has shape ", gradOutput.sizes(), ", expected ", im1.sizes());
    c10::DeviceGuard guard(im1.device());
    at::Tensor a = im1.contiguous(), b = im2.contiguous(), go = gradOutput.contiguous();
    if (want1) grad1.resize_({g.N, g.C, g.H, g.W});   // fully written, no fill_(0)
    if (want2) grad2.resize_({g.N, g.C, g.H, g.W});
    TORCH_CHECK((!want1 || grad1.is_contiguous()) && (!want2 || grad2.is_contiguous()), op, ": gradients must be contiguous");
    check_rci(fn2i_ssim_backward(a.data_ptr(), b.data_ptr(), go.data_ptr(), want1 ? grad1.data_ptr() : nullptr, want2 ? grad2.data_ptr() : nullptr,
                                 g.N, g.C, g.H, g.W, (int)md, (float)c1, (float)c2, (int)border, current_stream(im1)), op);
    return 1;
}

at::Tensor ssim_forward_alloc(at::Tensor &im1, at::Tensor &im2, int64_t md, double c1, double c2, int64_t border)
{
    check_inputs(im1, im2, md, c1, c2, border, "ssim_cuda.forward_alloc");
    c10::DeviceGuard guard(im1.device());
    at::Tensor output = unsized(im1);
    ssim_forward_hip(im1, im2, output, md, c1, c2, border);
    return output;
}

// an undefined tensor (None in Python) for a gradient that is not wanted
std::vector<at::Tensor> ssim_backward_alloc(at::Tensor &im1, at::Tensor &im2, at::Tensor &gradOutput, int64_t md, double c1, double c2,
                                            int64_t border, bool want1, bool want2)
{
    TORCH_CHECK(want1 || want2, "ssim_cuda.backward_alloc: neither gradient is wanted");
    check_inputs(im1, im2, md, c1, c2, border, "ssim_cuda.backward_alloc");
    c10::DeviceGuard guard(im1.device());
    at::Tensor g1 = want1 ? unsized(im1) : at::Tensor(), g2 = want2 ? unsized(im1) : at::Tensor();
    ssim_backward_hip(im1, im2, gradOutput, g1, g2, md, c1, c2, border, want1, want2);
    return {g1, g2};
}

// ---- autograd node on the C++ side, as census_cuda.apply: no Python between `apply` and the launch
struct SsimOp : public torch::autograd::Function<SsimOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &im1, const at::Tensor &im2, int64_t md, double c1, double c2, int64_t border)
    {
        ctx->save_for_backward({im1, im2});
        ctx->saved_data["md"] = md;
        ctx->saved_data["c1"] = c1;
        ctx->saved_data["c2"] = c2;
        ctx->saved_data["border"] = border;
        at::Tensor a = im1, b = im2;
        return ssim_forward_alloc(a, b, md, c1, c2, border);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "SSIMFunction.backward");
        auto saved = ctx->get_saved_variables();
        at::Tensor a = saved[0], b = saved[1], go = grad_outputs[0];
        const bool w1 = ctx->needs_input_grad(0), w2 = ctx->needs_input_grad(1);
        if (!w1 && !w2) return {at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
        auto g = ssim_backward_alloc(a, b, go, ctx->saved_data["md"].toInt(), ctx->saved_data["c1"].toDouble(), ctx->saved_data["c2"].toDouble(),
                                     ctx->saved_data["border"].toInt(), w1, w2);
        return {g[0], g[1], at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

at::Tensor ssim_apply(const at::Tensor &im1, const at::Tensor &im2, int64_t md, double c1, double c2, int64_t border)
{
    return SsimOp::apply(im1, im2, md, c1, c2, border);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "Structural-similarity distance: the SSIM photometric term of unsupervised flow, stereo and depth, gfx950 HIP kernels";
    m.def("apply", &ssim_apply, "SSIMFunction.apply: differentiable in im1 and im2, autograd node on the C++ side", py::arg("im1"), py::arg("im2"),
          py::arg("max_distance") = 1, py::arg("c1") = 1e-4, py::arg("c2") = 9e-4, py::arg("border") = 0);
    m.def("forward_alloc", &ssim_forward_alloc, "forward returning a freshly allocated N x C x H x W output", py::arg("im1"), py::arg("im2"),
          py::arg("max_distance") = 1, py::arg("c1") = 1e-4, py::arg("c2") = 9e-4, py::arg("border") = 0);
    m.def("backward_alloc", &ssim_backward_alloc, "backward returning freshly allocated gradients (im1, im2); None for one not wanted",
          py::arg("im1"), py::arg("im2"), py::arg("grad_output"), py::arg("max_distance") = 1, py::arg("c1") = 1e-4, py::arg("c2") = 9e-4,
          py::arg("border") = 0, py::arg("want1") = true, py::arg("want2") = true);
    m.def("forward", &ssim_forward_hip, "SSIM distance forward (HIP, gfx950); output is resized in place", py::arg("im1"), py::arg("im2"),
          py::arg("output"), py::arg("max_distance") = 1, py::arg("c1") = 1e-4, py::arg("c2") = 9e-4, py::arg("border") = 0);
    m.def("backward", &ssim_backward_hip, "SSIM distance backward (HIP, gfx950); the wanted gradients are resized in place", py::arg("im1"),
          py::arg("im2"), py::arg("grad_output"), py::arg("grad1"), py::arg("grad2"), py::arg("max_distance") = 1, py::arg("c1") = 1e-4,
          py::arg("c2") = 9e-4, py::arg("border") = 0, py::arg("want1") = true, py::arg("want2") = true);
    m.attr("MAX_DISTANCE") = (int)FN2I_MAX_DISTANCE;
    m.attr("BORDER_ZERO") = (int)FN2I_BORDER_ZERO;
    m.attr("BORDER_REFLECT") = (int)FN2I_BORDER_REFLECT;
    m.attr("TILE_H") = (int)FN2I_TILE_H;
    m.attr("TILE_W") = (int)FN2I_TILE_W;
}
