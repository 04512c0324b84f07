// ssim.h -- parameter block and launchers of the structural-similarity distance (ssim.hip), shared with the entry points of
// libflownet2_hip_ssim.so (capi_ssim.hip).  float32 throughout.
#pragma once
#include "fn2_common.h"

namespace fn2 {

struct SsimP {
    int planes, H, W;       // N C independent planes
    int tiles_x, tiles_y;   // FN2I_TILE_W x FN2I_TILE_H tiles per plane: the grid is planes tiles_x tiles_y workgroups
    int md;                 // 1, 2 or 3
    int reflect;            // border: 0 zero, 1 reflect
    int vec;                // every row of every staged tensor starts on 16 bytes: the tiles are staged with 16-byte loads
    float c1, c2;
};

// shape check: FN2_EINVAL, or FN2_EUNSUPPORTED for a plane, a plane count, a tensor or a grid beyond the launchers' limits
int ssim_make_params(SsimP &p, int N, int C, int H, int W);
// the parameters: md in 1..3, c1 and c2 finite and > 0, border in {0, 1}, reflect needs H > md and W > md
int ssim_set_options(SsimP &p, int md, float c1, float c2, int border);

int ssim_forward(const float *im1, const float *im2, float *out, SsimP p, hipStream_t s);
// g1 or g2 may be nullptr (not both): that gradient is not computed
int ssim_backward(const float *im1, const float *im2, const float *go, float *g1, float *g2, SsimP p, hipStream_t s);

} // namespace fn2
