// capi_smooth.hip -- C-ABI entry points of libflownet2_hip_smooth.so (include/flownet2_hip_smooth.h): the edge-aware smoothness term.
// Self-contained: links nothing of the other six libraries.  Every check comes before any launch, in the header's order.
#include "smooth.h"   // (brings flownet2_hip.h: the codes the smoothness header restates)
#include "../../include/flownet2_hip_smooth.h"

extern "C" int fn2m_abi_version(void) { return FN2M_ABI_VERSION; }

extern "C" int fn2m_smoothness_forward(const void *flow, const void *image, void *out, int N, int F, int C, int H, int W, int order,
                                       int edge_weighting, float alpha, float eps, void *stream)
{
    using namespace fn2;
    SmoothP p;
    int rc = smooth_make_params(p, N, F, C, H, W);
    if (rc != FN2_OK) return rc;
    if (N == 0) return FN2_OK;
    if (!flow || !image || !out) return FN2_EINVAL;
    if (!aligned(flow, 4) || !aligned(image, 4) || !aligned(out, 4)) return FN2_EALIGN;
    if ((rc = smooth_set_options(p, order, edge_weighting, alpha, eps)) != FN2_OK) return rc;
    return smooth_forward(static_cast<const float *>(flow), static_cast<const float *>(image), static_cast<float *>(out), p,
                          static_cast<hipStream_t>(stream));
}

extern "C" int fn2m_smoothness_backward(const void *flow, const void *image, const void *grad_out, void *grad_flow, int N, int F, int C,
                                        int H, int W, int order, int edge_weighting, float alpha, float eps, void *stream)
{
    using namespace fn2;
    SmoothP p;
    int rc = smooth_make_params(p, N, F, C, H, W);
    if (rc != FN2_OK) return rc;
    if (N == 0) return FN2_OK;
    if (!flow || !image || !grad_out || !grad_flow) return FN2_EINVAL;
    if (!aligned(flow, 4) || !aligned(image, 4) || !aligned(grad_out, 4) || !aligned(grad_flow, 4)) return FN2_EALIGN;
    if ((rc = smooth_set_options(p, order, edge_weighting, alpha, eps)) != FN2_OK) return rc;
    return smooth_backward(static_cast<const float *>(flow), static_cast<const float *>(image), static_cast<const float *>(grad_out),
                           static_cast<float *>(grad_flow), p, static_cast<hipStream_t>(stream));
}
