// splat_fixed.h -- the fixed-point helpers of ForwardWarp's deterministic forward (include/flownet2_hip_splat.h,
// fn2s_forward_warp_forward_det): the scale exponent of a plane from the bits of its maximum, a contribution as an int64, and a
// finished cell back to float.  Device only; included by forward_warp.hip alone.
#pragma once
#include <hip/hip_runtime.h>

namespace fn2 {

// what a plane's maximum (the bits of max |input|; their integer order is the order of the magnitudes, NaN above inf) says
enum { SPLAT_PLANE_ZERO = 0, SPLAT_PLANE_FINITE = 1, SPLAT_PLANE_BROKEN = 2 };

// E = frexp exponent of M (2^(E-1) <= M < 2^E, subnormals included) and s = 62 - E - K
__device__ __forceinline__ int splat_scale(unsigned m, int K, int &s)
{
    if (m == 0u) return SPLAT_PLANE_ZERO;
    if (m >= 0x7f800000u) return SPLAT_PLANE_BROKEN;
    const int E = m >= 0x00800000u ? (int)(m >> 23) - 126 : (32 - __clz((int)m)) - 149;
    s = 62 - E - K;
    return SPLAT_PLANE_FINITE;
}

// q = round-to-nearest-even(v 2^s): the scaling is exact in double (s may exceed fp32's exponent range), one rounding to int64;
// two's complement in an unsigned word, which atomicAdd wraps the same way
__device__ __forceinline__ unsigned long long splat_q(float v, int s) { return (unsigned long long)__double2ll_rn(ldexp((double)v, s)); }

// (float)((double)Q 2^-s): int64 -> double and double -> float, both round-to-nearest-even, subnormals kept
__device__ __forceinline__ float splat_unq(unsigned long long Q, int s) { return __double2float_rn(ldexp(__ll2double_rn((long long)Q), -s)); }

} // namespace fn2
