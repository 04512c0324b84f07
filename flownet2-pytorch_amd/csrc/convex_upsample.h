// convex_upsample.h -- parameter block and launchers of ConvexUpsample (convex_upsample.hip), shared with the entry points of
// libflownet2_hip_upsample.so (capi_upsample.hip).  float32 flow and output, float32 / float16 / bfloat16 mask.
#pragma once
#include "fn2_common.h"

namespace fn2 {

struct UpsampleP {
    int B, C, H, W;   // flow geometry; mask is B x 9 f^2 x H x W, out B x C x f H x f W
    int f;            // factor: 2, 4 or 8
    int tiles;        // FN2U_TILE-pixel tiles per row
    float scale;
};

// shape / parameter check: FN2_EINVAL, or FN2_EUNSUPPORTED for C > FN2U_MAX_CHANNELS, an output plane or a grid beyond 32-bit indices
int upsample_make_params(UpsampleP &p, int B, int C, int H, int W, int factor, float scale);

// mask_dtype: FN2_F32, FN2_F16 or FN2_BF16 (checked by the caller)
int upsample_forward(const float *flow, const void *mask, float *out, int mask_dtype, const UpsampleP &p, hipStream_t s);
// grad_mask and T (the workspace: B x C x 9 x H x W floats), then grad_flow gathered from T
int upsample_backward(const float *flow, const void *mask, const float *go, float *gflow, void *gmask, float *T, int mask_dtype,
                      const UpsampleP &p, hipStream_t s);

} // namespace fn2
