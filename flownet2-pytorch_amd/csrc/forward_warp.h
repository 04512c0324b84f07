// forward_warp.h -- parameter block and launchers of ForwardWarp (forward_warp.hip), shared with the entry points of
// libflownet2_hip_splat.so (capi_splat.hip).  float32 throughout.
#pragma once
#include "fn2_common.h"

namespace fn2 {

struct SplatP {
    int B, C, H, W;
    int chunks;             // 256-pixel chunks per plane (one lane per source pixel kernels)
    int tiles_x, tiles_y;   // FN2S_TILE_W x FN2S_TILE_H tiles per plane (tiled forward)
    int K;                  // ceil(log2(H W)) (deterministic forward)
    int groups_per_wg;      // tiled forward: channel groups a workgroup walks, and
    int group_runs;         // how many such runs cover the channels: the grid is B tiles_x tiles_y group_runs workgroups
};

// shape check: FN2_EINVAL, or FN2_EUNSUPPORTED for a plane, a plane count, a tensor or a grid beyond the launchers' limits
int splat_make_params(SplatP &p, int B, int C, int H, int W);
// bytes of the deterministic forward's workspace: the plane maxima (4 B each, rounded up to 256 B), then B C H W int64 cells
size_t splat_det_workspace_bytes(const SplatP &p);

// out is cleared on the stream first; tiled: the LDS-patch kernel, otherwise one lane per source pixel
int splat_forward(const float *in, const float *flow, float *out, const SplatP &p, bool tiled, hipStream_t s);
int splat_forward_det(const float *in, const float *flow, float *out, void *workspace, const SplatP &p, hipStream_t s);
// either gradient may be null (not both)
int splat_backward(const float *in, const float *flow, const float *go, float *gin, float *gflow, const SplatP &p, hipStream_t s);

} // namespace fn2
