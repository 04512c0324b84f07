// capi_splat.hip -- C-ABI entry points of libflownet2_hip_splat.so (include/flownet2_hip_splat.h): ForwardWarp.
// Self-contained: links nothing of the other four libraries.  Every check comes before any launch, in the header's order.
#include "forward_warp.h"   // (brings flownet2_hip.h: the codes the splat header restates)
#include "../../include/flownet2_hip_splat.h"

extern "C" int fn2s_abi_version(void) { return FN2S_ABI_VERSION; }

// FN2S_AUTO: the tiled kernel.  Measured 8 times the general kernel on smooth flows at both benchmark shapes, level with it or
// 8 % slower on random flows, and up to 1.55 times slower on flows of whole pixels (profiles/forward_warp_micro.json).
static bool auto_takes_tiled(const fn2::SplatP &) { return true; }

extern "C" int fn2s_forward_warp_forward(const void *input, const void *flow, void *out, int B, int C, int H, int W, int algo, void *stream)
{
    using namespace fn2;
    SplatP p;
    int rc = splat_make_params(p, B, C, H, W);
    if (rc != FN2_OK) return rc;
    if (B == 0) return FN2_OK;
    if (!input || !flow || !out) return FN2_EINVAL;
    if (!aligned(input, 4) || !aligned(flow, 4) || !aligned(out, 4)) return FN2_EALIGN;
    if (algo < FN2S_AUTO || algo > FN2S_TILED) return FN2_EINVAL;
    const bool tiled = algo == FN2S_TILED || (algo == FN2S_AUTO && auto_takes_tiled(p));
    return splat_forward(static_cast<const float *>(input), static_cast<const float *>(flow), static_cast<float *>(out), p, tiled,
                         static_cast<hipStream_t>(stream));
}

extern "C" size_t fn2s_forward_warp_forward_det_workspace_bytes(int B, int C, int H, int W)
{
    fn2::SplatP p;
    if (fn2::splat_make_params(p, B, C, H, W) != FN2_OK || B == 0) return 0;
    return fn2::splat_det_workspace_bytes(p);
}

extern "C" int fn2s_forward_warp_forward_det(const void *input, const void *flow, void *out, void *workspace, size_t workspace_bytes, int B,
                                             int C, int H, int W, void *stream)
{
    using namespace fn2;
    SplatP p;
    int rc = splat_make_params(p, B, C, H, W);
    if (rc != FN2_OK) return rc;
    if (B == 0) return FN2_OK;
    if (!input || !flow || !out || !workspace) return FN2_EINVAL;
    if (!aligned(input, 4) || !aligned(flow, 4) || !aligned(out, 4) || !aligned(workspace, 8)) return FN2_EALIGN;
    if (workspace_bytes < splat_det_workspace_bytes(p)) return FN2_EINVAL;
    return splat_forward_det(static_cast<const float *>(input), static_cast<const float *>(flow), static_cast<float *>(out), workspace, p,
                             static_cast<hipStream_t>(stream));
}

extern "C" int fn2s_forward_warp_backward(const void *input, const void *flow, const void *grad_out, void *grad_input, void *grad_flow, int B,
                                          int C, int H, int W, void *stream)
{
    using namespace fn2;
    SplatP p;
    int rc = splat_make_params(p, B, C, H, W);
    if (rc != FN2_OK) return rc;
    if (B == 0) return FN2_OK;
    if (!input || !flow || !grad_out || (!grad_input && !grad_flow)) return FN2_EINVAL;
    if (!aligned(input, 4) || !aligned(flow, 4) || !aligned(grad_out, 4) || !aligned(grad_input, 4) || !aligned(grad_flow, 4)) return FN2_EALIGN;
    return splat_backward(static_cast<const float *>(input), static_cast<const float *>(flow), static_cast<const float *>(grad_out),
                          static_cast<float *>(grad_input), static_cast<float *>(grad_flow), p, static_cast<hipStream_t>(stream));
}
