// resample2d_common.h -- device helpers shared by the warp kernels (resample2d.hip: float32; resample2d_lowp.hip: half / bfloat16).
#pragma once
#include "fn2_common.h"

namespace fn2 {

typedef float __attribute__((ext_vector_type(4))) f4;

struct ImgStrides { long b, c, h, w; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// int(floor(xf)) with CUDA's saturating float->int conversion (cvt.rzi.s32.f32; NaN -> 0).
__device__ __forceinline__ int f2i_sat(float v)
{
    if (!(v == v)) return 0;
    if (v >= 2147483520.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int)v;
}
__device__ __forceinline__ int d2i_sat(double v)
{
    if (!(v == v)) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (-2147483647 - 1);
    return (int)v;
}

// The forward's bilinear sample (resample2d_kernel.cu:56-59) as every kernel of resample2d.hip writes it out: weights in double from
// the fp32 alpha / beta ("1." literals), each term rounded to float, float accumulation from 0 in the order TL, TR, BL, BR.
__device__ __forceinline__ float bilinear_sample(float alpha, float beta, float i00, float i01, float i10, float i11)
{
    const double a = (double)alpha, be = (double)beta;
    float val = 0.0f;
    val = val + (float)(((1. - a) * (1. - be)) * (double)i00);
    val = val + (float)((a * (1. - be)) * (double)i01);
    val = val + (float)(((1. - a) * be) * (double)i10);
    val = val + (float)((a * be) * (double)i11);
    return val;
}

// One channel's terms of the flow gradient (resample2d_kernel.cu:172-177, :185-190), in the order resample_bwd_kernel adds them.
__device__ __forceinline__ void flow_grad_terms(float &out_dx, float &out_dy, float gam_x, float gam_y, float go, float iTL, float iTR,
                                                float iBL, float iBR)
{
    out_dy = out_dy + (gam_y * go) * iBL;
    out_dy = out_dy - (gam_y * go) * iTL;
    out_dy = out_dy + ((1 - gam_y) * go) * iBR;
    out_dy = out_dy - ((1 - gam_y) * go) * iTR;
    out_dx = out_dx + (gam_x * go) * iTR;
    out_dx = out_dx - (gam_x * go) * iTL;
    out_dx = out_dx + ((1 - gam_x) * go) * iBR;
    out_dx = out_dx - ((1 - gam_x) * go) * iBL;
}

} // namespace fn2
