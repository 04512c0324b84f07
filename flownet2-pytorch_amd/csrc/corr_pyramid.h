// corr_pyramid.h -- parameter block and launchers of the pyramid build (CorrPyramid; corr_pyramid.hip), shared with the entry
// points of libflownet2_hip_pyramid.so (capi_pyramid.hip).  float32 only.
#pragma once
#include "fn2_common.h"

#include "../../include/preview/flownet2_hip_pyramid.h"

namespace fn2 {

// Passed to the kernels BY VALUE: a captured launch keeps the level pointers and sizes it was given.
struct PyramidP {
    float *lvl[FN2Y_MAX_LEVELS];   // the levels (forward: written) or their gradients (fold: read; nullptr = missing)
    int L;                         // levels in use
    int B, C, H, W, H2, W2;        // level l is (B H W) x (H2 >> l) x (W2 >> l)
    float s;                       // (float)(1.0 / sqrt((double)C))
};

int pyramid_forward(const float *f1, const float *f2, const PyramidP &p, hipStream_t s);
int pyramid_fold(const PyramidP &p, float *G, hipStream_t s);

} // namespace fn2
