// corr1d.h -- parameter block and launchers of the horizontal-search correlation (Correlation1d; correlation_1d.hip), shared with
// the entry points of libflownet2_hip_ext.so (capi_ext.hip).
#pragma once
#include "fn2_common.h"

namespace fn2 {

struct Corr1dP {
    int B, C, H, W;            // input1 / input2 shape (NCHW)
    int pad, md, s1, s2, sd;   // pad_size, max_displacement, stride1, stride2, single_direction
    int dr, tmin, nOut, oH, oW;   // displacements t = tmin .. tmin + nOut - 1 (times s2); output channel o = t - tmin
};

int corr1d_output_shape(int H, int W, int pad, int md, int s1, int s2, int sd, int *nOut, int *oH, int *oW);
int corr1d_make_params(Corr1dP &p, int B, int C, int H, int W, int pad, int md, int s1, int s2, int sd);

// general kernels: any parameters, f32 / f16 / f64 / bf16
int corr1d_forward_general(const void *in1, const void *in2, void *out, int dtype, const Corr1dP &p, hipStream_t s);
int corr1d_backward_general(const void *in1, const void *in2, const void *gout, void *g1, void *g2, int dtype, const Corr1dP &p,
                            hipStream_t s);

// LDS-tiled kernels with the general kernels' bits: s1 = s2 = 1, pad == md, nOut <= 81, f32 / f16 / bf16, shapes inside the
// launcher's 32-bit offsets and grid limits.  Outside that they decline (FN2_EUNSUPPORTED, nothing launched).
bool corr1d_tiled_applicable(int dtype, const Corr1dP &p);
bool corr1d_forward_pays(const Corr1dP &p);   // what AUTO asks before it takes the tiled FORWARD (measured gate)
int corr1d_forward_tiled(const void *in1, const void *in2, void *out, int dtype, const Corr1dP &p, hipStream_t s);
int corr1d_backward_tiled(const void *in1, const void *in2, const void *gout, void *g1, void *g2, int dtype, const Corr1dP &p,
                          hipStream_t s);

} // namespace fn2
