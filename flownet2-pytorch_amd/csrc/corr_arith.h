// corr_arith.h -- the arithmetic of the parameter-general correlation kernels (correlation_direct.hip), shared with the kernels
// that promise its bits (correlation_dense.hip): one definition, so the two cannot drift apart.
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

} // namespace fn2
