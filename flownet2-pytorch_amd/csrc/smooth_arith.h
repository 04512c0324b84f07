// smooth_arith.h -- the arithmetic of the edge-aware smoothness term (include/flownet2_hip_smooth.h): the edge weight, the flow
// differences, the robust function and its derivative.  Host and device: every kernel of smooth.hip uses it, and a plain C++
// program can include it to test it (tests/test_smoothness_host.py compiles it under the undefined-behaviour sanitizer).
// fp32 throughout, every operation rounded on its own (the library is built with -ffp-contract=off; nothing here can contract).
//
// exp2, the square root and the reciprocal square root are the hardware's (v_exp_f32, v_sqrt_f32, v_rsq_f32: within 1 ulp, one
// 8-cycle issue each) on the device and libm's on the host.  v_exp_f32 returns 0 for a result below 2^-126.
//
// Summation orders, followed by the kernels:
//   channels    e = ((a_0 + a_1) + a_2) FN2M_THIRD for C = 3, e = a_0 for C = 1
//   flow        sum_f rho = ((rho_0 + rho_1) + rho_2) + rho_3, ascending f, starting from rho_0
//   gather      per direction g = t[q - 1] - t[q] (order 1), g = (t[q - 2] - 2 t[q - 1]) + t[q] (order 2); grad = g_x + g_y
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FN2M_HD __host__ __device__ __forceinline__
#else
#define FN2M_HD static inline
#endif

#define FN2M_LOG2E 1.44269504f   // fl32(log2(e)): exp(-e) = exp2(-(e FN2M_LOG2E))
#define FN2M_THIRD 0.333333343f  // fl32(1 / 3): the mean over three channels

FN2M_HD float smooth_exp2(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(v);
#else
    return exp2f(v);
#endif
}

FN2M_HD float smooth_sqrt(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(v);
#else
    return sqrtf(v);
#endif
}

FN2M_HD float smooth_rsq(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(v);
#else
    return 1.0f / sqrtf(v);
#endif
}

// one channel's share of the edge measure from its image difference dI = I[p + k] - I[p]: |alpha dI| or (alpha dI)^2
FN2M_HD float smooth_edge_term(float dI, float alpha, int gaussian)
{
    const float t = alpha * dI;
    return gaussian ? t * t : fabsf(t);
}

FN2M_HD float smooth_mean3(float a0, float a1, float a2) { return ((a0 + a1) + a2) * FN2M_THIRD; }

// w = exp(-e), e >= 0; e = +0 gives exp2(-0) = 1 exactly
FN2M_HD float smooth_weight(float e) { return smooth_exp2(-(e * FN2M_LOG2E)); }

// first and second difference of three consecutive flow values
FN2M_HD float smooth_d1(float f0, float f1) { return f1 - f0; }
FN2M_HD float smooth_d2(float f0, float f1, float f2) { return (f2 - f1) - (f1 - f0); }

// rho(d) = sqrt(d^2 + eps^2), eps2 = fl32(eps eps); eps2 = 0 is the L1 form, taken exactly: rho = |d|
FN2M_HD float smooth_rho(float d, float eps2)
{
    const float s = d * d + eps2;
    return eps2 == 0.0f ? fabsf(d) : smooth_sqrt(s);
}

// rho'(d) = d rsq(d^2 + eps^2); eps2 = 0: sign(d), exactly 0 at d = 0
FN2M_HD float smooth_drho(float d, float eps2)
{
    const float s = d * d + eps2;
    const float sign = d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : 0.0f;
    return eps2 == 0.0f ? sign : d * smooth_rsq(s);
}
