// splat_taps.h -- the tap computation of ForwardWarp (include/flownet2_hip_splat.h): where a source pixel lands, whether it
// takes part at all, and its four bilinear weights.  Host and device: every kernel of forward_warp.hip uses it, and a plain C++
// program can include it to test it (tests/test_forward_warp_host.py compiles it under the undefined-behaviour sanitizer).
// fp32 throughout, every operation rounded on its own (the library is built with -ffp-contract=off; nothing here can contract).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FN2S_HD __host__ __device__ __forceinline__
#else
#define FN2S_HD static inline
#endif

struct SplatTaps {
    int valid;                  // 0: the pixel contributes nothing and gets zero gradients; everything below is 0 then
    int x0, y0;                 // tap (dy, dx) is cell (y0 + dy, x0 + dx); -1 <= x0 <= W - 1, -1 <= y0 <= H - 1
    float ax, ay, bx, by;       // fx - x0, fy - y0, 1 - ax, 1 - ay
    float w00, w01, w10, w11;   // w_dydx: bx by, ax by, bx ay, ax ay
};

// the landing position of source coordinate i along one axis: fl32(fl32(i) + flow)
FN2S_HD float splat_pos(int i, float flow) { return (float)i + flow; }

// The test is made on the floats, before any conversion to int, and written so that NaN fails it: a valid position lies in
// (-1, n) with n < 2^31, so its floor converts exactly.
FN2S_HD SplatTaps splat_taps(float fx, float fy, int W, int H)
{
    SplatTaps t;
    t.valid = (fx > -1.0f) && (fx < (float)W) && (fy > -1.0f) && (fy < (float)H);
    t.x0 = t.y0 = 0;
    t.ax = t.ay = t.bx = t.by = t.w00 = t.w01 = t.w10 = t.w11 = 0.0f;
    if (!t.valid) return t;
    const float flx = floorf(fx), fly = floorf(fy);
    t.x0 = (int)flx;
    t.y0 = (int)fly;
    t.ax = fx - flx;
    t.ay = fy - fly;
    t.bx = 1.0f - t.ax;
    t.by = 1.0f - t.ay;
    t.w00 = t.bx * t.by;
    t.w01 = t.ax * t.by;
    t.w10 = t.bx * t.ay;
    t.w11 = t.ax * t.ay;
    return t;
}
