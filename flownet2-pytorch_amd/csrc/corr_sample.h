// corr_sample.h -- parameter block and launchers of the pyramid lookup (CorrSample; corr_sample.hip), shared with the entry
// points of libflownet2_hip_sample.so (capi_sample.hip).  float32 only.
#pragma once
#include "fn2_common.h"

#include "../../include/preview/flownet2_hip_sample.h"

namespace fn2 {

// Passed to the kernels BY VALUE: a captured launch keeps the level pointers and sizes it was given.
struct SampleP {
    float *lvl[FN2P_MAX_LEVELS];   // the levels (forward: read) or their gradients (backward: written)
    int H2[FN2P_MAX_LEVELS], W2[FN2P_MAX_LEVELS];
    int L;         // levels in use
    int B, H, W;   // coords / out geometry
    int r;         // radius; D = 2 r + 1
};

int sample_forward(const float *co, float *out, const SampleP &p, hipStream_t s);
int sample_backward(const float *co, const float *go, const SampleP &p, hipStream_t s);

} // namespace fn2
