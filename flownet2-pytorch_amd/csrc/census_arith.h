// census_arith.h -- the arithmetic of the ternary census distance (include/flownet2_hip_census.h): the grey intensity, the soft
// sign f and its derivative, the robust distance h and its derivative.  Host and device: every kernel of census.hip uses it, and
// a plain C++ program can include it to test it (tests/test_census_host.py compiles it under the undefined-behaviour sanitizer).
// fp32 throughout, every operation rounded on its own (the library is built with -ffp-contract=off; nothing here can contract).
//
// The reciprocal square root and the reciprocal are the hardware's (v_rsq_f32, v_rcp_f32: within 1 ulp, one 8-cycle issue each)
// on the device and the correctly rounded quotient on the host.  Their arguments are >= 0.81 and >= 0.1: no subnormal, no zero.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FN2C_HD __host__ __device__ __forceinline__
#else
#define FN2C_HD static inline
#endif

#define FN2C_GREY_R 0.2989f
#define FN2C_GREY_G 0.5870f
#define FN2C_GREY_B 0.1140f
#define FN2C_F_EPS 0.81f   // f(x) = x / sqrt(0.81 + x^2)
#define FN2C_H_EPS 0.1f    // h(d) = d^2 / (0.1 + d^2)

FN2C_HD float census_rsq(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(v);
#else
    return 1.0f / sqrtf(v);
#endif
}

FN2C_HD float census_rcp(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(v);
#else
    return 1.0f / v;
#endif
}

// ((r 0.2989 + g 0.5870) + b 0.1140) scale, in this order
FN2C_HD float census_grey3(float r, float g, float b, float scale) { return ((r * FN2C_GREY_R + g * FN2C_GREY_G) + b * FN2C_GREY_B) * scale; }
FN2C_HD float census_grey1(float v, float scale) { return v * scale; }

// r(x) = 1 / sqrt(0.81 + x^2): f = x r and f' = 0.81 r^3 share it
FN2C_HD float census_r(float x) { return census_rsq(FN2C_F_EPS + x * x); }
FN2C_HD float census_f(float x) { return x * census_r(x); }
FN2C_HD float census_df_r(float r) { return FN2C_F_EPS * ((r * r) * r); }
FN2C_HD float census_df(float x) { return census_df_r(census_r(x)); }

// q(d) = 1 / (0.1 + d^2): h = d^2 q and h' = 0.2 d q^2 share it
FN2C_HD float census_h(float d)
{
    const float d2 = d * d;
    return d2 * census_rcp(FN2C_H_EPS + d2);
}
FN2C_HD float census_dh(float d)
{
    const float q = census_rcp(FN2C_H_EPS + d * d);
    return ((2.0f * FN2C_H_EPS) * d) * (q * q);
}

// one tap of the forward: h(f(x1) - f(x2))
FN2C_HD float census_tap(float x1, float x2) { return census_h(census_f(x1) - census_f(x2)); }
