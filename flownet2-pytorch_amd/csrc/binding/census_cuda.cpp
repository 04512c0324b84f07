// census_cuda.cpp -- pybind module `census_cuda`: the ternary census distance (include/flownet2_hip_census.h) on the caller's
// current HIP stream.  Not one of the reference's modules: it links libflownet2_hip_census.so only.
// forward / backward take caller-provided tensors and resize them in place; *_alloc return fresh tensors; apply is the
// differentiable op with its autograd node on the C++ side, which asks only for the gradients that are needed.  Everything is
// float32.  No global state.
#include "binding_common.h"
#include "flownet2_hip_census.h"

using namespace fn2b;

// the status text of libflownet2_hip_census.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rcc(int rc, const char *op) { check_status(STATUS_CENSUS, rc, op); }

struct Geo {
    int N, C, H, W;
};

// the arguments first, then where the tensors live: a wrong shape, dtype or parameter is reported as such on any device
static Geo check_inputs(const at::Tensor &im1, const at::Tensor &im2, int64_t md, double scale, const char *op)
{
    TORCH_CHECK(im1.defined() && im2.defined(), op, ": im1 or im2 is undefined");
    TORCH_CHECK(im1.dim() == 4 && im2.dim() == 4, op, ": im1 and im2 must be 4-D (N, C, H, W); add the missing dimensions with [None]");
    TORCH_CHECK(im1.sizes() == im2.sizes(), op, ": im2 ", im2.sizes(), " must have the shape of im1 ", im1.sizes());
    TORCH_CHECK(im1.size(1) == 1 || im1.size(1) == 3, op, ": the images have ", im1.size(1), " channels, expected 1 (grey) or 3 (RGB)");
    TORCH_CHECK(md >= 1 && md <= FN2C_MAX_DISTANCE, op, ": max_distance ", md, " is not 1, 2 or 3");
    TORCH_CHECK(std::isfinite((float)scale), op, ": scale ", scale, " is not a finite float");
    check_f32(im1, op, "im1");
    check_f32(im2, op, "im2");
    check_gpu(im1, op, "im1");
    check_gpu(im2, op, "im2");
    TORCH_CHECK(im2.device() == im1.device(), op, ": im2 is on ", im2.device(), ", expected ", im1.device());
    return Geo{(int)im1.size(0), (int)im1.size(1), (int)im1.size(2), (int)im1.size(3)};
}

int census_forward_hip(at::Tensor &im1, at::Tensor &im2, at::Tensor &output, int64_t md, double scale, bool normalize)
{
    const char *op = "census_cuda.forward";
    const Geo g = check_inputs(im1, im2, md, scale, op);
    check_same(im1, output, op, "output");
    c10::DeviceGuard guard(im1.device());
    at::Tensor a = im1.contiguous(), b = im2.contiguous();
    output.resize_({g.N, 1, g.H, g.W});   // fully written by the kernel, no fill_(0)
    TORCH_CHECK(output.is_contiguous(), op, ": output must be contiguous");
    check_rcc(fn2c_census_forward(a.data_ptr(), b.data_ptr(), output.data_ptr(), g.N, g.C, g.H, g.W, (int)md, (float)scale, normalize ? 1 : 0,
                                  current_stream(im1)), op);
    return 1;
}

// want1 / want2: which gradients to compute; the other tensor is left as it is
int census_backward_hip(at::Tensor &im1, at::Tensor &im2, at::Tensor &gradOutput, at::Tensor &grad1, at::Tensor &grad2, int64_t md, double scale,
                        bool normalize, bool want1, bool want2)
{
    const char *op = "census_cuda.backward";
    TORCH_CHECK(want1 || want2, op, ": neither gradient is wanted");
    const Geo g = check_inputs(im1, im2, md, scale, op);
    check_same(im1, gradOutput, op, "gradOutput");
    if (want1) check_same(im1, grad1, op, "grad1");
    if (want2) check_same(im1, grad2, op, "grad2");
    TORCH_CHECK(gradOutput.dim() == 4 && gradOutput.size(0) == g.N && gradOutput.size(1) == 1 && gradOutput.size(2) == g.H && gradOutput.size(3) == g.W,
                op, ": gradOutput has shape ", gradOutput.sizes(), ", expected [", g.N, ", 1, ", g.H, ", ", g.W, "]");
    c10::DeviceGuard guard(im1.device());
    at::Tensor a = im1.contiguous(), b = im2.contiguous(), go = gradOutput.contiguous();
    if (want1) grad1.resize_({g.N, g.C, g.H, g.W});   // fully written, no fill_(0)
    if (want2) grad2.resize_({g.N, g.C, g.H, g.W});
    TORCH_CHECK((!want1 || grad1.is_contiguous()) && (!want2 || grad2.is_contiguous()), op, ": gradients must be contiguous");
    check_rcc(fn2c_census_backward(a.data_ptr(), b.data_ptr(), go.data_ptr(), want1 ? grad1.data_ptr() : nullptr, want2 ? grad2.data_ptr() : nullptr,
                                   g.N, g.C, g.H, g.W, (int)md, (float)scale, normalize ? 1 : 0, current_stream(im1)), op);
    return 1;
}

at::Tensor census_forward_alloc(at::Tensor &im1, at::Tensor &im2, int64_t md, double scale, bool normalize)
{
    check_inputs(im1, im2, md, scale, "census_cuda.forward_alloc");
    c10::DeviceGuard guard(im1.device());
    at::Tensor output = unsized(im1);
    census_forward_hip(im1, im2, output, md, scale, normalize);
    return output;
}

// an undefined tensor (None in Python) for a gradient that is not wanted
std::vector<at::Tensor> census_backward_alloc(at::Tensor &im1, at::Tensor &im2, at::Tensor &gradOutput, int64_t md, double scale, bool normalize,
                                              bool want1, bool want2)
{
    TORCH_CHECK(want1 || want2, "census_cuda.backward_alloc: neither gradient is wanted");
    check_inputs(im1, im2, md, scale, "census_cuda.backward_alloc");
    c10::DeviceGuard guard(im1.device());
    at::Tensor g1 = want1 ? unsized(im1) : at::Tensor(), g2 = want2 ? unsized(im1) : at::Tensor();
    census_backward_hip(im1, im2, gradOutput, g1, g2, md, scale, normalize, want1, want2);
    return {g1, g2};
}

// ---- autograd node on the C++ side, as forward_warp_cuda.apply: no Python between `apply` and the launch
struct CensusOp : public torch::autograd::Function<CensusOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &im1, const at::Tensor &im2, int64_t md, double scale, bool normalize)
    {
        ctx->save_for_backward({im1, im2});
        ctx->saved_data["md"] = md;
        ctx->saved_data["scale"] = scale;
        ctx->saved_data["normalize"] = normalize;
        at::Tensor a = im1, b = im2;
        return census_forward_alloc(a, b, md, scale, normalize);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "CensusFunction.backward");
        auto saved = ctx->get_saved_variables();
        at::Tensor a = saved[0], b = saved[1], go = grad_outputs[0];
        const bool w1 = ctx->needs_input_grad(0), w2 = ctx->needs_input_grad(1);
        if (!w1 && !w2) return {at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
        auto g = census_backward_alloc(a, b, go, ctx->saved_data["md"].toInt(), ctx->saved_data["scale"].toDouble(),
                                       ctx->saved_data["normalize"].toBool(), w1, w2);
        return {g[0], g[1], at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

at::Tensor census_apply(const at::Tensor &im1, const at::Tensor &im2, int64_t md, double scale, bool normalize)
{
    return CensusOp::apply(im1, im2, md, scale, normalize);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "Ternary census distance: the photometric term of unsupervised optical flow, gfx950 HIP kernels";
    m.def("apply", &census_apply, "CensusFunction.apply: differentiable in im1 and im2, autograd node on the C++ side", py::arg("im1"),
          py::arg("im2"), py::arg("max_distance") = 3, py::arg("scale") = 255.0, py::arg("normalize") = true);
    m.def("forward_alloc", &census_forward_alloc, "forward returning a freshly allocated N x 1 x H x W output", py::arg("im1"), py::arg("im2"),
          py::arg("max_distance") = 3, py::arg("scale") = 255.0, py::arg("normalize") = true);
    m.def("backward_alloc", &census_backward_alloc, "backward returning freshly allocated gradients (im1, im2); None for one not wanted",
          py::arg("im1"), py::arg("im2"), py::arg("grad_output"), py::arg("max_distance") = 3, py::arg("scale") = 255.0,
          py::arg("normalize") = true, py::arg("want1") = true, py::arg("want2") = true);
    m.def("forward", &census_forward_hip, "census distance forward (HIP, gfx950); output is resized in place", py::arg("im1"), py::arg("im2"),
          py::arg("output"), py::arg("max_distance") = 3, py::arg("scale") = 255.0, py::arg("normalize") = true);
    m.def("backward", &census_backward_hip, "census distance backward (HIP, gfx950); the wanted gradients are resized in place", py::arg("im1"),
          py::arg("im2"), py::arg("grad_output"), py::arg("grad1"), py::arg("grad2"), py::arg("max_distance") = 3, py::arg("scale") = 255.0,
          py::arg("normalize") = true, py::arg("want1") = true, py::arg("want2") = true);
    m.attr("MAX_DISTANCE") = (int)FN2C_MAX_DISTANCE;
}
