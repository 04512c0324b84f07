// census.h -- parameter block and launchers of the ternary census distance (census.hip), shared with the entry points of
// libflownet2_hip_census.so (capi_census.hip).  float32 throughout.
#pragma once
#include "fn2_common.h"

namespace fn2 {

struct CensusP {
    int N, C, H, W;
    int tiles_x, tiles_y;   // FN2C_TILE_W x FN2C_TILE_H tiles per plane: the grid is N tiles_x tiles_y workgroups
    int md;                 // max_distance, 1..3
    float scale;            // grey = weighted channels * scale
    float w;                // fl32(1 / (2 md + 1)^2) if normalize else 1
};

// shape check: FN2_EINVAL, or FN2_EUNSUPPORTED for a plane, a plane count, a tensor or a grid beyond the launchers' limits
int census_make_params(CensusP &p, int N, int C, int H, int W);
// the parameters, checked last: C in {1, 3}, md in {1, 2, 3}, scale finite
int census_set_options(CensusP &p, int md, float scale, int normalize);

int census_forward(const float *im1, const float *im2, float *out, const CensusP &p, hipStream_t s);
// either gradient may be null (not both)
int census_backward(const float *im1, const float *im2, const float *go, float *g1, float *g2, const CensusP &p, hipStream_t s);

} // namespace fn2
