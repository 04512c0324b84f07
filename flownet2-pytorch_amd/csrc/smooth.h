// smooth.h -- parameter block and launchers of the edge-aware smoothness term (smooth.hip), shared with the entry points of
// libflownet2_hip_smooth.so (capi_smooth.hip).  float32 throughout.
#pragma once
#include "fn2_common.h"

namespace fn2 {

struct SmoothP {
    int N, F, C, H, W;
    int tiles_x, tiles_y;   // FN2M_TILE_W x FN2M_TILE_H tiles per plane: the grid is N tiles_x tiles_y workgroups
    int order;              // k, 1 or 2
    int gaussian;           // edge_weighting: 0 exponential, 1 gaussian
    int vec;                // every row of every tensor starts on 16 bytes: the tiles are staged with 16-byte loads
    float alpha;
    float eps2;             // fl32(eps eps)
};

// shape check: FN2_EINVAL, or FN2_EUNSUPPORTED for a plane, a plane count, a tensor or a grid beyond the launchers' limits
int smooth_make_params(SmoothP &p, int N, int F, int C, int H, int W);
// the parameters, checked last: C in {1, 3}, F in 1..4, order in {1, 2}, edge in {0, 1}, alpha and eps finite and >= 0
int smooth_set_options(SmoothP &p, int order, int edge, float alpha, float eps);

int smooth_forward(const float *flow, const float *image, float *out, SmoothP p, hipStream_t s);
int smooth_backward(const float *flow, const float *image, const float *go, float *gflow, SmoothP p, hipStream_t s);

} // namespace fn2
