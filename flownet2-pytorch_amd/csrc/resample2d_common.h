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

// The forward's bilinear sample (resample2d_kernel.cu:56-59), the one copy the kernels of both files call: weights in double from the
// fp32 alpha / beta ("1." literals), each term rounded to float, float accumulation from 0 in the order TL, TR, BL, BR.  Kernels that
// gather several channels with one position form the weights once (bilinear_weights) and pass them on.  One term is NOT the reference's
// arithmetic to the bit: its BR term `(alpha) * (beta) * I` (:59) has no double literal and is formed in fp32 with two roundings, where
// w11 here is the double product like the other three (one rounding, closer to the exact value).  tests/test_gpu_warp_contract.py pins
// this sequence bit for bit and counts the elements that differ from the reference's.
struct BilinearW { double w00, w01, w10, w11; };
__device__ __forceinline__ BilinearW bilinear_weights(float alpha, float beta)
{
    const double a = (double)alpha, be = (double)beta;
    return BilinearW{(1. - a) * (1. - be), a * (1. - be), (1. - a) * be, a * be};
}
__device__ __forceinline__ float bilinear_sample(const BilinearW &w, float i00, float i01, float i10, float i11)
{
    float val = 0.0f;
    val = val + (float)(w.w00 * (double)i00);
    val = val + (float)(w.w01 * (double)i01);
    val = val + (float)(w.w10 * (double)i10);
    val = val + (float)(w.w11 * (double)i11);
    return val;
}
__device__ __forceinline__ float bilinear_sample(float alpha, float beta, float i00, float i01, float i10, float i11)
{
    return bilinear_sample(bilinear_weights(alpha, beta), i00, i01, i10, i11);
}

// The sampling position of one pixel on an image of the flow's size: the forward's corners and weights (resample2d_kernel.cu:45-52,
// :66-67) -- in nearest mode all four corners are the nearest pixel -- or, BWD, the corners the flow gradient gathers (always the
// bilinear ones, :163-166).
struct WarpPos { int xL, xR, yT, yB; float alpha, beta; };
template <bool BWD> __device__ __forceinline__ WarpPos warp_pos(int x, int y, float dx, float dy, int H, int W, int bilinear)
{
    WarpPos q;
    const float xf = (float)x + dx, yf = (float)y + dy;
    const float fx = floorf(xf), fy = floorf(yf);
    q.alpha = xf - fx; q.beta = yf - fy;
    if (BWD || bilinear) {
        q.xL = clampi(f2i_sat(fx), 0, W - 1); q.xR = clampi(f2i_sat(fx + 1.0f), 0, W - 1);
        q.yT = clampi(f2i_sat(fy), 0, H - 1); q.yB = clampi(f2i_sat(fy + 1.0f), 0, H - 1);
    } else {
        q.xL = q.xR = clampi(d2i_sat(floor((double)xf + 0.5)), 0, W - 1);
        q.yT = q.yB = clampi(d2i_sat(floor((double)yf + 0.5)), 0, H - 1);
    }
    return q;
}
// The forward's corners on an image of its own size Hi x Wi, as the float32 kernels take them: clamped with the flow's dims (:49-52),
// then to the image (defensive); alpha / beta are written in bilinear mode only (nearest mode never reads them: the caller's zeros
// stay).  Not warp_pos with Hi == H: the second clamp is not folded away, and plain references keep the float32 kernels' code where
// a returned WarpPos does not (its adjacent alpha, beta get packed arithmetic).
__device__ __forceinline__ void warp_fwd_corners(int x, int y, float dx, float dy, int H, int W, int Hi, int Wi, int bilinear, int &xL,
                                                 int &xR, int &yT, int &yB, float &alpha, float &beta)
{
    const float xf = (float)x + dx, yf = (float)y + dy;
    if (bilinear) {
        const float fx = floorf(xf), fy = floorf(yf);
        alpha = xf - fx; beta = yf - fy;
        xL = clampi(clampi(f2i_sat(fx), 0, W - 1), 0, Wi - 1);
        xR = clampi(clampi(f2i_sat(fx + 1.0f), 0, W - 1), 0, Wi - 1);
        yT = clampi(clampi(f2i_sat(fy), 0, H - 1), 0, Hi - 1);
        yB = clampi(clampi(f2i_sat(fy + 1.0f), 0, H - 1), 0, Hi - 1);
    } else {   // floor(xf + 0.5) in double
        xL = xR = clampi(clampi(d2i_sat(floor((double)xf + 0.5)), 0, W - 1), 0, Wi - 1);
        yT = yB = clampi(clampi(d2i_sat(floor((double)yf + 0.5)), 0, H - 1), 0, Hi - 1);
    }
}
// the forward's value from the gathered corners.  Backward, nearest mode: the nearest pixel is the corner alpha / beta >= 0.5 select
// (floor(xf + 0.5) = floor(xf) + (alpha >= 0.5), clamped like the corner), as resample_bwd_c3x recomputes it.
template <bool BWD> __device__ __forceinline__ float warp_value(const WarpPos &q, int bilinear, float i00, float i01, float i10, float i11)
{
    if (bilinear) return bilinear_sample(q.alpha, q.beta, i00, i01, i10, i11);
    if (!BWD) return i00;
    return q.alpha >= 0.5f ? (q.beta >= 0.5f ? i11 : i01) : (q.beta >= 0.5f ? i10 : i00);
}

// What the backward kernels derive from one pixel's flow before any clamp (resample2d_kernel.cu:105-106, :163-169, :182): the raw corner
// indices int(floor) and int(floor + 1), the scatter's alpha / beta by TRUNCATION (xf - int(xf)), and the floor fractions fa / fb (the
// forward's alpha / beta): the flow gradient's gamma is 1 - fa for d/d(dy) (:169) and 1 - fb for d/d(dx) (:182).  Plain references, as
// warp_fwd_corners.
__device__ __forceinline__ void warp_bwd_pos(int x, int y, float dx, float dy, int &ixL, int &ixR, int &iyT, int &iyB, float &alpha,
                                             float &beta, float &fa, float &fb)
{
    const float xf = (float)x + dx, yf = (float)y + dy;
    const float fx = floorf(xf), fy = floorf(yf);
    ixL = f2i_sat(fx); ixR = f2i_sat(fx + 1.0f); iyT = f2i_sat(fy); iyB = f2i_sat(fy + 1.0f);
    alpha = xf - (float)f2i_sat(xf); beta = yf - (float)f2i_sat(yf);
    fa = xf - fx; fb = yf - fy;
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

// grid of the one-lane-per-element kernels (grid-stride loops): at most 2048 workgroups of 256 threads
static inline unsigned stream_grid(long nthreads)
{
    long blocks = (nthreads + 255) / 256;
    const long cap = 256L * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

} // namespace fn2
