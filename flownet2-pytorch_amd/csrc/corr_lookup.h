// corr_lookup.h -- parameter block and launchers of the correlation lookup (CorrLookup; corr_lookup.hip), shared with the entry
// points of libflownet2_hip_lookup.so (capi_lookup.hip).  float32 only.
#pragma once
#include "fn2_common.h"

namespace fn2 {

struct LookupP {
    int B, C, H, W;   // fmap1 (and coords, out) geometry
    int H2, W2;       // fmap2 geometry: any pyramid level
    int r;            // radius; D = 2 r + 1
    float scale;
};

// shape / parameter check: FN2_EINVAL, or FN2_EUNSUPPORTED for a plane or a grid beyond the launchers' 32-bit indices
int lookup_make_params(LookupP &p, int B, int C, int H, int W, int H2, int W2, int radius, float scale);

// general kernels: any valid input, 0 <= r <= 8
int lookup_forward_general(const float *f1, const float *f2, const float *co, float *out, const LookupP &p, hipStream_t s);
// LDS-staged kernels with the general kernels' bits: r <= 4
int lookup_forward_staged(const float *f1, const float *f2, const float *co, float *out, const LookupP &p, hipStream_t s);
// grad_fmap1 (gather; general or staged) and grad_fmap2 (memset + atomic scatter, always the general kernel)
int lookup_backward(const float *f1, const float *f2, const float *co, const float *go, float *g1, float *g2, const LookupP &p,
                    bool staged, hipStream_t s);

bool lookup_staged_applicable(const LookupP &p);   // r <= FN2L_STAGED_MAX_RADIUS
bool lookup_staged_pays(const LookupP &p);         // what AUTO asks (measured; include/flownet2_hip_lookup.h)

} // namespace fn2
