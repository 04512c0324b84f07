// binding_common.h -- what the ten pybind modules share (host C++, no kernels): the checks on tensors, the status checks of the
// main library (fn2_strerror) and of the sibling libraries (binding_status.h), the current stream, the double-backward guard of
// the autograd nodes, and the preamble of the two modules that take an equally shaped pair of inputs.  Each module keeps its own
// check_inputs, entry points, autograd node and PYBIND11_MODULE block, and forwards to the C ABI of the one library it links
// (include/flownet2_hip*.h) on the caller's current HIP stream.  The three drop-in modules keep the reference's module names and
// positional signatures (correlation_cuda.cc:169-172, resample2d_cuda.cc:28-31, channelnorm_cuda.cc:27-30).
#pragma once
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>

#include <initializer_list>

#include "binding_status.h"
#include "flownet2_hip.h"

namespace fn2b {

using torch::autograd::AutogradContext;   // every module has an autograd node on the C++ side
using torch::autograd::variable_list;

inline int dtype_of(const at::Tensor &t, const char *op)
{
    switch (t.scalar_type()) {
    case at::kFloat: return FN2_F32;
    case at::kHalf: return FN2_F16;
    case at::kDouble: return FN2_F64;
    case at::kBFloat16: return FN2_BF16;
    default: TORCH_CHECK(false, op, ": unsupported dtype ", t.scalar_type(), " (float, half, double or bfloat16 expected)");
    }
    return -1;
}

// The HIP kernels are the only implementation: there is no CPU path to fall back to.
inline void check_gpu(const at::Tensor &t, const char *op, const char *name)
{
    TORCH_CHECK(t.defined(), op, ": ", name, " is undefined");
    TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be a GPU (HIP) tensor; this extension has no CPU implementation");
}

inline void check_same(const at::Tensor &a, const at::Tensor &b, const char *op, const char *nb)
{
    check_gpu(b, op, nb);
    TORCH_CHECK(a.device() == b.device(), op, ": ", nb, " is on ", b.device(), ", expected ", a.device());
    TORCH_CHECK(a.scalar_type() == b.scalar_type(), op, ": ", nb, " has dtype ", b.scalar_type(), ", expected ",
                a.scalar_type());
}

inline void check_f32(const at::Tensor &t, const char *op, const char *name)
{
    TORCH_CHECK(t.scalar_type() == at::kFloat, op, ": ", name, " must be float32, got ", t.scalar_type(), ": convert it with .float()");
}

// the main library (the modules that link libflownet2_hip.so)
inline void check_rc(int rc, const char *op)
{
    // reference: launcher returns 0 -> AT_ERROR("CUDA call failed") (correlation_cuda.cc:81-83)
    TORCH_CHECK(rc == FN2_OK, op, ": HIP call failed: ", fn2_strerror(rc), " (code ", rc, ")");
}

// a sibling library (STATUS_* of binding_status.h); nothing is formatted unless the call failed
inline void check_status(const StatusText &lib, int rc, const char *op)
{
    if (rc != FN2_OK) TORCH_CHECK(false, status_message(lib, op, rc));
}

// PyTorch-ROCm presents HIP devices as device type "cuda"; the masquerading accessor is the one
// that matches the tensors' device type (the plain c10::hip guard/stream classes expect type "hip").
inline void *current_stream(const at::Tensor &t)
{
    return static_cast<void *>(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream());
}

// torch.use_deterministic_algorithms(True), warn_only included: the scattering passes then take the fixed-point entry points
inline bool deterministic() { return at::globalContext().deterministicAlgorithms(); }
// their workspace, straight from the caching allocator of the current device (at::empty would fill it under the deterministic
// flag; the entry point clears it on the stream itself); released to the allocator when the DataPtr goes, as a temporary tensor is
inline c10::DataPtr det_workspace(size_t bytes) { return c10::GetAllocator(c10::DeviceType::CUDA)->allocate(bytes); }

// an empty tensor (numel 0) like `t`: a result for an entry point to resize in place, or the placeholder of one that is not wanted
inline at::Tensor unsized(const at::Tensor &t) { return at::empty({0}, t.options()); }

// first line of an autograd node's backward; `op`: the node's name, as in "CorrelationFunction.backward"
inline void check_once_differentiable(const variable_list &grads, const char *op)
{
    for (const auto &g : grads)
        TORCH_CHECK(!(g.defined() && g.requires_grad() && at::GradMode::is_enabled()), op,
                    ": the backward of this layer is a HIP kernel and not differentiable a second time (create_graph=True)");
}

// ---- correlation_cuda and correlation1d_cuda: two equally shaped 4-D inputs and a cost volume
struct PairGeo {
    int dt, B, C, H, W;
    int nOut, oH, oW;   // zero until the caller's output_shape call has filled them in
};

struct NamedTensor {
    const at::Tensor &t;
    const char *name;
};

// input1 on the GPU; input2 and `others` on its device and of its dtype, in this order; then 4-D and equal sizes.
// forward_wording: the two messages of `forward`, which name the shapes; else the one message of the other entry points.
inline PairGeo check_pair(const at::Tensor &input1, const at::Tensor &input2, std::initializer_list<NamedTensor> others, const char *op,
                          bool forward_wording = false)
{
    check_gpu(input1, op, "input1");
    check_same(input1, input2, op, "input2");
    for (const NamedTensor &o : others) check_same(input1, o.t, op, o.name);
    if (forward_wording) {
        TORCH_CHECK(input1.dim() == 4 && input2.dim() == 4, op, ": inputs must be 4-D (N, C, H, W)");
        TORCH_CHECK(input1.sizes() == input2.sizes(), op, ": input1 ", input1.sizes(), " and input2 ", input2.sizes(),
                    " must have the same shape");
    } else {
        TORCH_CHECK(input1.dim() == 4 && input1.sizes() == input2.sizes(), op, ": inputs must be 4-D and equally shaped");
    }
    return PairGeo{dtype_of(input1, op), (int)input1.size(0), (int)input1.size(1), (int)input1.size(2), (int)input1.size(3), 0, 0, 0};
}

inline void check_grad_output(const at::Tensor &gradOutput, const PairGeo &g, const char *op)
{
    TORCH_CHECK(gradOutput.dim() == 4 && gradOutput.size(0) == g.B && gradOutput.size(1) == g.nOut && gradOutput.size(2) == g.oH &&
                    gradOutput.size(3) == g.oW,
                op, ": gradOutput has shape ", gradOutput.sizes(), ", expected [", g.B, ", ", g.nOut, ", ", g.oH, ", ", g.oW, "]");
}

} // namespace fn2b
