// corr_sample1d.h -- parameter block and launchers of the 1-D pyramid lookup (CorrSample1d; corr_sample1d.hip), shared with the
// entry points of libflownet2_hip_sample1d.so (capi_sample1d.hip).  float32 only.
#pragma once
#include "fn2_common.h"

#include "../../include/staging/flownet2_hip_sample1d.h"

namespace fn2 {

// consecutive pixels of one batch item per workgroup.  Forward: TILE (2 r + 2) must be a multiple of 64 for every r and divide 256.
constexpr int SAMPLE1D_TILE_FORWARD = 32, SAMPLE1D_TILE_BACKWARD = 32;

// Passed to the kernels BY VALUE: a captured launch keeps the level pointers and sizes it was given.
struct Sample1dP {
    float *lvl[FN2H_MAX_LEVELS];   // the levels (forward: read) or their gradients (backward: written)
    int W2[FN2H_MAX_LEVELS];
    int L;           // levels in use
    int B, H, W;     // coords / out geometry
    int r;           // radius; D = 2 r + 1
    long long cbs;   // coords_x's batch stride in elements, >= H W
};

int sample1d_forward(const float *cx, float *out, const Sample1dP &p, hipStream_t s);
int sample1d_backward(const float *cx, const float *go, const Sample1dP &p, hipStream_t s);

} // namespace fn2
