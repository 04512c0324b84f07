// corr_arith.h -- the arithmetic of the parameter-general correlation kernels (correlation_direct.hip, corr1d_*_general in
// correlation_1d.hip), shared with the tiled kernels that promise its bits (corr_tiled.h, correlation_dense.hip,
// correlation_1d.hip): one definition, so they cannot drift apart.  Also the one host helper both general launches share,
// stream_grid(nthreads, cap_blocks).
#pragma once
#include <type_traits>

#include "fn2_common.h"

namespace fn2 {

template <typename T> struct Acc { typedef float type; };
template <> struct Acc<double> { typedef double type; };

// one product of the forward: in T (:124), except for bf16 (exact in fp32)
template <typename T> __device__ __forceinline__ float fwd_prod(T a, T b)
{
    if constexpr (std::is_same<T, bf16_t>::value) return (float)a * (float)b;
    else return (float)(T)(a * b);
}

// the channel sum of one (pixel, displacement) pair of the forward, pa / pb the two pixels in channel 0: four partial sums over
// the channels c = 0,1,2,3 (mod 4) in ascending order (4 independent chains for ILP), the C % 4 leftover channels appended to
// the first, then (s0 + s1) + (s2 + s3)
template <typename T> __device__ __forceinline__ float fwd_channel_sum(const T *pa, const T *pb, int C, long HW)
{
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int c = 0;
    for (; c + 4 <= C; c += 4) {
        s0 += fwd_prod<T>(pa[(long)(c + 0) * HW], pb[(long)(c + 0) * HW]);
        s1 += fwd_prod<T>(pa[(long)(c + 1) * HW], pb[(long)(c + 1) * HW]);
        s2 += fwd_prod<T>(pa[(long)(c + 2) * HW], pb[(long)(c + 2) * HW]);
        s3 += fwd_prod<T>(pa[(long)(c + 3) * HW], pb[(long)(c + 3) * HW]);
    }
    for (; c < C; ++c) s0 += fwd_prod<T>(pa[(long)c * HW], pb[(long)c * HW]);
    return (s0 + s1) + (s2 + s3);
}

// grid of the general kernels: one lane of a 256-thread block per element, grid-stride beyond cap_blocks
static inline unsigned stream_grid(long nthreads, long cap_blocks)
{
    long blocks = (nthreads + 255) / 256;
    if (blocks > cap_blocks) blocks = cap_blocks;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

} // namespace fn2
