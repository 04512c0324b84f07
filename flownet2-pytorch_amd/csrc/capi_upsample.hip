// capi_upsample.hip -- C-ABI entry points of libflownet2_hip_upsample.so (include/flownet2_hip_upsample.h): ConvexUpsample.
// Self-contained: links nothing of the other three libraries.  Every check comes before any launch, in the header's order.
#include "convex_upsample.h"   // (brings flownet2_hip.h: the codes and element types the upsample header restates)
#include "../../include/flownet2_hip_upsample.h"

extern "C" int fn2u_abi_version(void) { return FN2U_ABI_VERSION; }

namespace {
bool mask_dtype_ok(int dt) { return dt == FN2_F32 || dt == FN2_F16 || dt == FN2_BF16; }
} // namespace

extern "C" int fn2u_convex_upsample_forward(const void *flow, const void *mask, void *out, int mask_dtype, int B, int C, int H, int W,
                                            int factor, float scale, void *stream)
{
    using namespace fn2;
    if (!mask_dtype_ok(mask_dtype)) return FN2_EDTYPE;
    UpsampleP p;
    int rc = upsample_make_params(p, B, C, H, W, factor, scale);
    if (rc != FN2_OK) return rc;
    if (B == 0) return FN2_OK;
    if (!flow || !mask || !out) return FN2_EINVAL;
    if (!aligned(flow, 4) || !aligned(mask, dtype_size(mask_dtype)) || !aligned(out, 4)) return FN2_EALIGN;
    return upsample_forward(static_cast<const float *>(flow), mask, static_cast<float *>(out), mask_dtype, p, static_cast<hipStream_t>(stream));
}

extern "C" size_t fn2u_convex_upsample_backward_workspace_bytes(int B, int C, int H, int W)
{
    fn2::UpsampleP p;
    if (fn2::upsample_make_params(p, B, C, H, W, 2, 1.f) != FN2_OK) return 0;
    return (size_t)9 * sizeof(float) * B * C * H * W;
}

extern "C" int fn2u_convex_upsample_backward(const void *flow, const void *mask, const void *grad_out, void *grad_flow, void *grad_mask,
                                             void *workspace, int mask_dtype, int B, int C, int H, int W, int factor, float scale, void *stream)
{
    using namespace fn2;
    if (!mask_dtype_ok(mask_dtype)) return FN2_EDTYPE;
    UpsampleP p;
    int rc = upsample_make_params(p, B, C, H, W, factor, scale);
    if (rc != FN2_OK) return rc;
    if (B == 0) return FN2_OK;
    if (!flow || !mask || !grad_out || !grad_flow || !grad_mask) return FN2_EINVAL;
    const size_t ms = dtype_size(mask_dtype);
    if (!aligned(flow, 4) || !aligned(mask, ms) || !aligned(grad_out, 4) || !aligned(grad_flow, 4) || !aligned(grad_mask, ms) ||
        !aligned(workspace, 4))
        return FN2_EALIGN;
    if (!workspace) return FN2_EINVAL;
    return upsample_backward(static_cast<const float *>(flow), mask, static_cast<const float *>(grad_out), static_cast<float *>(grad_flow),
                             grad_mask, static_cast<float *>(workspace), mask_dtype, p, static_cast<hipStream_t>(stream));
}
