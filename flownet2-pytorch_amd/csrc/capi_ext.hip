// capi_ext.hip -- C-ABI entry points of libflownet2_hip_ext.so (include/flownet2_hip_ext.h): layers that are not among the
// reference's three and therefore live outside the drop-in boundary of libflownet2_hip.so.  Self-contained: links nothing of the
// main library.
#include "corr1d.h"   // (brings flownet2_hip.h: the codes and element types the ext header restates)
#include "../../include/flownet2_hip_ext.h"

extern "C" int fn2x_abi_version(void) { return FN2X_ABI_VERSION; }

extern "C" int fn2x_correlation1d_output_shape(int H, int W, int pad_size, int max_displacement, int stride1, int stride2,
                                               int single_direction, int *nOut, int *oH, int *oW)
{
    return fn2::corr1d_output_shape(H, W, pad_size, max_displacement, stride1, stride2, single_direction, nOut, oH, oW);
}

extern "C" int fn2x_correlation1d_forward(const void *in1, const void *in2, void *out, int dtype, int B, int C, int H, int W,
                                          int pad_size, int max_displacement, int stride1, int stride2, int single_direction,
                                          int algo, void *stream)
{
    using namespace fn2;
    const size_t es = dtype_size(dtype);
    if (!es) return FN2_EDTYPE;
    Corr1dP p;
    int rc = corr1d_make_params(p, B, C, H, W, pad_size, max_displacement, stride1, stride2, single_direction);
    if (rc != FN2_OK) return rc;
    if (B == 0) return FN2_OK;
    if (!in1 || !in2 || !out) return FN2_EINVAL;
    if (!aligned(in1, es) || !aligned(in2, es) || !aligned(out, es)) return FN2_EALIGN;
    if (algo < FN2X_CORR1D_AUTO || algo > FN2X_CORR1D_TILED) return FN2_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool tiled_ok = corr1d_tiled_applicable(dtype, p);   // decided before anything is launched
    if (algo == FN2X_CORR1D_TILED) return tiled_ok ? corr1d_forward_tiled(in1, in2, out, dtype, p, s) : FN2_EUNSUPPORTED;
    if (algo == FN2X_CORR1D_AUTO && tiled_ok && corr1d_forward_pays(p)) return corr1d_forward_tiled(in1, in2, out, dtype, p, s);
    return corr1d_forward_general(in1, in2, out, dtype, p, s);
}

extern "C" int fn2x_correlation1d_backward(const void *in1, const void *in2, const void *grad_out, void *grad_in1, void *grad_in2,
                                           int dtype, int B, int C, int H, int W, int pad_size, int max_displacement, int stride1,
                                           int stride2, int single_direction, int algo, void *stream)
{
    using namespace fn2;
    const size_t es = dtype_size(dtype);
    if (!es) return FN2_EDTYPE;
    Corr1dP p;
    int rc = corr1d_make_params(p, B, C, H, W, pad_size, max_displacement, stride1, stride2, single_direction);
    if (rc != FN2_OK) return rc;
    if (stride1 != 1) return FN2_EUNSUPPORTED;   // as the 2-D layer: the backward is defined for stride1 = 1 only
    if (B == 0) return FN2_OK;
    if (!in1 || !in2 || !grad_out || !grad_in1 || !grad_in2) return FN2_EINVAL;
    if (!aligned(in1, es) || !aligned(in2, es) || !aligned(grad_out, es) || !aligned(grad_in1, es) || !aligned(grad_in2, es))
        return FN2_EALIGN;
    if (algo < FN2X_CORR1D_AUTO || algo > FN2X_CORR1D_TILED) return FN2_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool tiled_ok = corr1d_tiled_applicable(dtype, p);
    if (algo == FN2X_CORR1D_TILED && !tiled_ok) return FN2_EUNSUPPORTED;
    // the tiled backward splits the channels over workgroups: AUTO takes it at every size
    if (algo != FN2X_CORR1D_GENERAL && tiled_ok) return corr1d_backward_tiled(in1, in2, grad_out, grad_in1, grad_in2, dtype, p, s);
    return corr1d_backward_general(in1, in2, grad_out, grad_in1, grad_in2, dtype, p, s);
}
