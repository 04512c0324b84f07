// fn2_common.h -- shared device/host helpers for libflownet2_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/flownet2_hip.h"

#define FN2_WAVE 64

namespace fn2 {

typedef _Float16 half_t;
typedef __bf16 bf16_t;

static inline int launch_status()
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? FN2_OK : (int)e;
}

static inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// Zero fill of n 32-bit words at a 4-byte aligned address, as a kernel: words up to the first 16-byte boundary, 16-byte stores, the
// last words.  The libraries clear what their atomics add into with this, not with hipMemsetAsync.  Observed, not explained: captured
// into a hipGraph through torch.cuda.graph on this runtime, the hipMemsetAsync of these buffers did not clear them on replay
// (tests/test_gpu_pipelines.py: the scatters then added onto uninitialised memory or onto the last replay's sums; tests/
// test_gpu_capi_graph.py: the MultiScale ticket counter and the empty batch's sums), while the same call outside a graph always did;
// why the memset node fails has not been found.  A kernel node replays like the kernels around it.  No library enqueues a memset node.
template <int = 0> __global__ void __launch_bounds__(256) zero_fill_kernel(unsigned *p, size_t n)
{
    const size_t to16 = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4;
    const size_t head = to16 < n ? to16 : n, nv = (n - head) / 4, done = head + 4 * nv;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    uint4 *v = reinterpret_cast<uint4 *>(p + head);
    for (size_t i = tid; i < nv; i += stride) v[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid < head) p[tid] = 0u;
    if (tid < n - done) p[done + tid] = 0u;
}

// Enqueue the clear of `bytes` bytes (a multiple of 4) at p (4-byte aligned) on s.
static inline int zero_fill_async(void *p, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return FN2_OK;
    if (bytes % 4 != 0 || !aligned(p, 4)) return FN2_EALIGN;
    const size_t n = bytes / 4, want = (n / 4 + 255) / 256 + 1;
    hipLaunchKernelGGL(zero_fill_kernel<0>, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, s, static_cast<unsigned *>(p), n);
    return launch_status();
}

static inline size_t dtype_size(int dtype)
{
    switch (dtype) {
    case FN2_F32: return 4;
    case FN2_F16: return 2;
    case FN2_F64: return 8;
    case FN2_BF16: return 2;
    default: return 0;
    }
}

// Store of a finished output element / vector (written once, read by a LATER kernel): agent scope (sc1) -- written through the
// XCD's L2 as it is issued.  The eight L2s are not coherent with each other, so everything a kernel wrote must be in memory when
// it ends; left dirty (a plain store) the outputs are flushed in one burst at the end of the kernel, which the next kernel of the
// stream waits for.  Measured inside bench.py's step (scripts/gpu_bench_ab.sh, same box, two rounds): ChannelNorm backward 11.4 ->
// 9.7 us, forward 8.0 -> 7.5, Resample2d forward 21.7 -> 21.4, step 0.1976 -> 0.1953 ms (non-temporal stores instead: 0.1948, but
// ChannelNorm forward 8.6 us); the correlation kernels' rows carry the same hint on their buffer stores (-5 % of the step).
template <class V> __device__ __forceinline__ void store_out(V *p, V v)
{
#if defined(FN2_ABL_OUTTEMPORAL)   // timing ablation: plain stores
    *p = v;
#elif defined(FN2_ABL_OUTNT)       // timing ablation: non-temporal stores
    __builtin_nontemporal_store(v, p);
#else
    // (s_nop: a store of more than 64 bits needs a wait state before its data registers may be overwritten; the compiler
    // provides it for its own instructions, not for inline assembly -- cf. correlation_f16x2.hip)
    if constexpr (sizeof(V) == 16) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (sizeof(V) == 8) asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (sizeof(V) == 4) asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    else *p = v;
#endif
}

// The two 16-bit matrix operand types (half, bfloat16) of the single-product correlation kernels: the 8-element fragment of
// v_mfma_f32_16x16x32_{f16,bf16} (same lane layout, same cycles, same C/D layout on gfx950) and the packed conversion of two fp32
// results (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN).
template <class E> struct Op16;
template <> struct Op16<half_t> {
    typedef half_t v8 __attribute__((ext_vector_type(8)));
    typedef half_t v2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float __attribute__((ext_vector_type(4)))
    mfma(v8 a, v8 b, float __attribute__((ext_vector_type(4))) c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ unsigned pk(float a, float b)
    {
        return __builtin_bit_cast(unsigned, __builtin_convertvector((float __attribute__((ext_vector_type(2)))){a, b}, v2));
    }
};
template <> struct Op16<bf16_t> {
    typedef bf16_t v8 __attribute__((ext_vector_type(8)));
    typedef bf16_t v2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float __attribute__((ext_vector_type(4)))
    mfma(v8 a, v8 b, float __attribute__((ext_vector_type(4))) c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ unsigned pk(float a, float b)
    {
        return __builtin_bit_cast(unsigned, __builtin_convertvector((float __attribute__((ext_vector_type(2)))){a, b}, v2));
    }
};

// ChannelNorm's gradient of one element (channelnorm_kernel.cu:93):
// static_cast<float>(gO) * static_cast<float>(x) / (static_cast<float>(out) + 1e-9) -- float product, double divide, rounded to float.
__device__ __forceinline__ float chnorm_grad(float go, float x, float o)
{
    const float prod = go * x;
    return (float)((double)prod / ((double)o + 1e-9));
}

// XCD-aware remap of a 1-D block index: consecutive logical tiles land on the same XCD
// (hardware dispatches block b to XCD b % 8), so neighbouring tiles share one L2.
// Bijective for any grid size (cdna guide 5 "XCD swizzle must be bijective").
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblk)
{
    const unsigned NX = 8;
    const unsigned q = nblk / NX, r = nblk % NX;
    const unsigned xcd = bid % NX, idx = bid / NX;
    const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

} // namespace fn2
