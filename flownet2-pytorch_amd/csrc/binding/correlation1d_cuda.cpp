// correlation1d_cuda.cpp -- pybind module `correlation1d_cuda`: the horizontal-search cost volume of stereo networks
// (Correlation1d; include/flownet2_hip_ext.h) on the caller's current HIP stream.  Not one of the reference's modules: it links
// libflownet2_hip_ext.so only.  forward / backward take caller-provided tensors and resize them in place, like correlation_cuda;
// *_alloc return fresh tensors; apply is the differentiable op with its autograd node on the C++ side.
#include "binding_common.h"
#include "flownet2_hip_ext.h"

using namespace fn2b;

// the status text of libflownet2_hip_ext.so (binding_status.h): this module does not link the library fn2_strerror lives in
static void check_rc1d(int rc, const char *op) { check_status(STATUS_EXT, rc, op); }

int correlation1d_forward_hip(at::Tensor &input1, at::Tensor &input2, at::Tensor &output, int pad_size, int max_displacement,
                              int stride1, int stride2, int single_direction)
{
    const char *op = "correlation1d_cuda.forward";
    PairGeo g = check_pair(input1, input2, {{output, "output"}}, op, true);
    check_rc1d(fn2x_correlation1d_output_shape(g.H, g.W, pad_size, max_displacement, stride1, stride2, single_direction, &g.nOut, &g.oH, &g.oW), op);
    const auto [dt, B, C, H, W, nOut, oH, oW] = g;
    c10::DeviceGuard guard(input1.device());
    at::Tensor a = input1.contiguous(), b = input2.contiguous();
    output.resize_({B, nOut, oH, oW});   // fully written by the kernel, no fill_(0)
    TORCH_CHECK(output.is_contiguous(), op, ": output must be contiguous");
    check_rc1d(fn2x_correlation1d_forward(a.data_ptr(), b.data_ptr(), output.data_ptr(), dt, B, C, H, W, pad_size, max_displacement,
                                          stride1, stride2, single_direction, FN2X_CORR1D_AUTO, current_stream(input1)), op);
    return 1;
}

int correlation1d_backward_hip(at::Tensor &input1, at::Tensor &input2, at::Tensor &gradOutput, at::Tensor &gradInput1,
                               at::Tensor &gradInput2, int pad_size, int max_displacement, int stride1, int stride2,
                               int single_direction)
{
    const char *op = "correlation1d_cuda.backward";
    PairGeo g = check_pair(input1, input2, {{gradOutput, "gradOutput"}, {gradInput1, "gradInput1"}, {gradInput2, "gradInput2"}}, op);
    check_rc1d(fn2x_correlation1d_output_shape(g.H, g.W, pad_size, max_displacement, stride1, stride2, single_direction, &g.nOut, &g.oH, &g.oW), op);
    const auto [dt, B, C, H, W, nOut, oH, oW] = g;
    check_grad_output(gradOutput, g, op);
    c10::DeviceGuard guard(input1.device());
    at::Tensor a = input1.contiguous(), b = input2.contiguous(), go = gradOutput.contiguous();
    gradInput1.resize_({B, C, H, W});   // fully written, no fill_(0)
    gradInput2.resize_({B, C, H, W});
    TORCH_CHECK(gradInput1.is_contiguous() && gradInput2.is_contiguous(), op, ": gradInputs must be contiguous");
    check_rc1d(fn2x_correlation1d_backward(a.data_ptr(), b.data_ptr(), go.data_ptr(), gradInput1.data_ptr(), gradInput2.data_ptr(), dt,
                                           B, C, H, W, pad_size, max_displacement, stride1, stride2, single_direction,
                                           FN2X_CORR1D_AUTO, current_stream(input1)), op);
    return 1;
}

at::Tensor correlation1d_forward_alloc(at::Tensor &input1, at::Tensor &input2, int pad_size, int max_displacement, int stride1,
                                       int stride2, int single_direction)
{
    check_gpu(input1, "correlation1d_cuda.forward_alloc", "input1");
    c10::DeviceGuard guard(input1.device());
    at::Tensor output = unsized(input1);
    correlation1d_forward_hip(input1, input2, output, pad_size, max_displacement, stride1, stride2, single_direction);
    return output;
}

std::vector<at::Tensor> correlation1d_backward_alloc(at::Tensor &input1, at::Tensor &input2, at::Tensor &gradOutput, int pad_size,
                                                     int max_displacement, int stride1, int stride2, int single_direction)
{
    check_gpu(input1, "correlation1d_cuda.backward_alloc", "input1");
    c10::DeviceGuard guard(input1.device());
    at::Tensor g1 = unsized(input1), g2 = unsized(input1);
    correlation1d_backward_hip(input1, input2, gradOutput, g1, g2, pad_size, max_displacement, stride1, stride2, single_direction);
    return {g1, g2};
}

// ---- autograd node on the C++ side, as correlation_cuda.apply: no Python between `apply` and the launch
struct Correlation1dOp : public torch::autograd::Function<Correlation1dOp> {
    static at::Tensor forward(AutogradContext *ctx, const at::Tensor &input1, const at::Tensor &input2, int64_t pad_size,
                              int64_t max_displacement, int64_t stride1, int64_t stride2, int64_t single_direction)
    {
        ctx->save_for_backward({input1, input2});
        ctx->saved_data["p"] = std::vector<int64_t>{pad_size, max_displacement, stride1, stride2, single_direction};
        at::Tensor a = input1, b = input2;
        return correlation1d_forward_alloc(a, b, (int)pad_size, (int)max_displacement, (int)stride1, (int)stride2, (int)single_direction);
    }

    static variable_list backward(AutogradContext *ctx, variable_list grad_outputs)
    {
        check_once_differentiable(grad_outputs, "Correlation1dFunction.backward");
        auto saved = ctx->get_saved_variables();
        const auto p = ctx->saved_data["p"].toIntVector();
        at::Tensor a = saved[0], b = saved[1], go = grad_outputs[0];
        auto g = correlation1d_backward_alloc(a, b, go, (int)p[0], (int)p[1], (int)p[2], (int)p[3], (int)p[4]);
        return {g[0], g[1], at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

at::Tensor correlation1d_apply(const at::Tensor &input1, const at::Tensor &input2, int64_t pad_size, int64_t max_displacement,
                               int64_t stride1, int64_t stride2, int64_t single_direction)
{
    return Correlation1dOp::apply(input1, input2, pad_size, max_displacement, stride1, stride2, single_direction);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "Correlation1d: horizontal-search cost volume for stereo networks, gfx950 HIP kernels";
    m.def("apply", &correlation1d_apply, "Correlation1dFunction.apply: differentiable, autograd node on the C++ side", py::arg("input1"),
          py::arg("input2"), py::arg("pad_size") = 0, py::arg("max_displacement") = 0, py::arg("stride1") = 1, py::arg("stride2") = 1,
          py::arg("single_direction") = 0);
    m.def("forward_alloc", &correlation1d_forward_alloc, "forward returning a freshly allocated output");
    m.def("backward_alloc", &correlation1d_backward_alloc, "backward returning freshly allocated gradients");
    m.def("forward", &correlation1d_forward_hip, "Correlation1d forward (HIP, gfx950); output is resized in place");
    m.def("backward", &correlation1d_backward_hip, "Correlation1d backward (HIP, gfx950); the gradients are resized in place");
}
