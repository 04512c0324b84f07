// capi.hip -- C-ABI entry points of libflownet2_hip.so that are not tied to one kernel file:
// error strings, shape math and the correlation dispatcher (include/flownet2_hip.h).
//
// The dispatcher is the table kCorrRows below: one row per kernel -- the algo values that select it, its domain and its launcher
// per direction, the alignment the dispatcher itself asks for -- in the order FN2_CORR_AUTO tries them.  corr_plan lists the rows
// a call selects that admit it (domain, alignment; forward: the batch stride's divisor and AUTO's gate), corr_dispatch runs them.
// FN2_CORR_AUTO goes on to the next row when a launcher declines (FN2_EUNSUPPORTED / FN2_EALIGN, nothing launched).  Any other algo
// plans the first admitted row it selects and returns that launcher's code as it is, or FN2_EUNSUPPORTED if there is none.  A debug
// variant (fn2_debug.h) names its row: 9000 DENSE, forward >= 5000 / backward >= 6000 F16X2, every other value MFMA_F32.
#include <math.h>

#include "corr_params.h"
#include "fn2_debug.h"


extern "C" const char *fn2_strerror(int code)
{
    switch (code) {
    case FN2_OK: return "ok";
    case FN2_EINVAL: return "flownet2_hip: invalid shape or parameter";
    case FN2_EDTYPE: return "flownet2_hip: dtype not supported by this op";
    case FN2_EALIGN: return "flownet2_hip: pointer not aligned to its element size";
    case FN2_EUNSUPPORTED: return "flownet2_hip: parameter combination the reference leaves undefined";
    default: break;
    }
    if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
    return "flownet2_hip: unknown error";
}

extern "C" int fn2_abi_version(void) { return FN2_ABI_VERSION; }

// correlation_cuda.cc:19-34
extern "C" int fn2_correlation_output_shape(int H, int W, int pad_size, int kernel_size, int max_displacement,
                                            int stride1, int stride2, int *nOut, int *oH, int *oW)
{
    if (H < 1 || W < 1 || pad_size < 0 || kernel_size < 1 || max_displacement < 0 || stride1 < 1 || stride2 < 1)
        return FN2_EINVAL;
    const int kernel_radius = (kernel_size - 1) / 2;
    const int border_radius = kernel_radius + max_displacement;
    const int pH = H + 2 * pad_size, pW = W + 2 * pad_size;
    const int d = (max_displacement / stride2) * 2 + 1;
    const int oh = (int)ceilf((float)(pH - 2 * border_radius) / (float)stride1);
    const int ow = (int)ceilf((float)(pW - 2 * border_radius) / (float)stride1);
    if (oh < 1 || ow < 1) return FN2_EINVAL;
    if (nOut) *nOut = d * d;
    if (oH) *oH = oh;
    if (oW) *oW = ow;
    return FN2_OK;
}

namespace fn2 {
namespace {

enum { FWD = 0, BWD = 1 };
struct CorrRow {                       // kCorrRows[FN2_CORR_KERNEL_x] (fn2_debug.h) is the row of kernel x
    unsigned algos;                    // bit a: algo a selects the row
    CorrPredicate *domain[2];          // [FWD], [BWD]; null: every call
    CorrLauncher *launch[2];
    int align[2], out_bs_div;          // bytes in1, in2 and out / grad_out must be aligned to (0: no rule here); forward: divisor of out_batch_stride
    bool align_grads;                  // backward: grad_in1 and grad_in2 as well
    bool (*auto_gate)(const CorrP &);  // forward under FN2_CORR_AUTO only: is the kernel worth taking?
};
#define FN2_ALGO(a) (1u << FN2_CORR_##a)
constexpr CorrRow kCorrRows[FN2_CORR_KERNEL_COUNT] = {
    /* H16 */ {FN2_ALGO(AUTO) | FN2_ALGO(MFMA_F16X2), {corr_f16_fwd_applicable, corr_f16_bwd_applicable},
               {corr_forward_f16, corr_backward_f16}, {0, 0}, 1, false, nullptr},
    /* F16X2 */ {FN2_ALGO(AUTO) | FN2_ALGO(MFMA_F16X2), {corr_f16x2_applicable, corr_bwd_f16x2_applicable},
                 {corr_forward_f16x2, corr_backward_f16x2}, {16, 16}, 4, true, nullptr},
    /* MFMA_F32 */ {FN2_ALGO(AUTO) | FN2_ALGO(MFMA_F32) | FN2_ALGO(MFMA_BF16X3), {corr_mfma_f32_applicable, corr_bwd_mfma_f32_applicable},
                    {corr_forward_mfma_f32, corr_backward_mfma_f32}, {8, 8}, 2, false, nullptr},
    /* F64 */ {FN2_ALGO(AUTO), {corr_mfma_f64_applicable, corr_mfma_f64_applicable},
               {corr_forward_mfma_f64, corr_backward_mfma_f64}, {16, 16}, 2, false, nullptr},
    /* DENSE */ {FN2_ALGO(AUTO), {corr_dense_applicable, corr_dense_applicable},
                 {corr_forward_dense, corr_backward_dense}, {0, 0}, 1, false, corr_dense_forward_pays},
    /* DIRECT */ {FN2_ALGO(AUTO) | FN2_ALGO(DIRECT), {nullptr, nullptr}, {corr_forward_direct, corr_backward_direct}, {0, 0}, 1, false, nullptr},
};
#undef FN2_ALGO

// How many rows corr_dispatch would try (the first `max` in ids[]; 0: an empty batch), or the code the call ends with before any launch
int corr_plan(int dir, const CorrCall &c, int algo, bool debug_variant, int *ids, int max)
{
    const void *ptrs[5] = {c.in1, c.in2, dir == FWD ? c.out : c.gout, c.g1, c.g2};
    const int nptrs = dir == FWD ? 3 : 5;
    if (c.p.B == 0) return 0;
    for (int i = 0; i < nptrs; ++i) if (!ptrs[i]) return FN2_EINVAL;
    for (int i = 0; i < nptrs; ++i) if (!aligned(ptrs[i], dtype_size(c.dtype))) return FN2_EALIGN;
    // profiling instantiations (wrong or partial outputs by design) are only reachable through fn2_debug_* (fn2_debug.h)
    if (!debug_variant && (algo < FN2_CORR_AUTO || algo > FN2_CORR_MFMA_F16X2)) return FN2_EINVAL;
    const bool walk = !debug_variant && algo == FN2_CORR_AUTO;
    const int named = algo == FN2_DEBUG_CORR_DENSE ? FN2_CORR_KERNEL_DENSE   // a debug variant names its row
                      : algo >= (dir == FWD ? 5000 : 6000) ? FN2_CORR_KERNEL_F16X2 : FN2_CORR_KERNEL_MFMA_F32;
    int n = 0;
    for (int id = 0; id < FN2_CORR_KERNEL_COUNT && (walk || n == 0); ++id) {
        const CorrRow &r = kCorrRows[id];
        const size_t a = r.align[dir];
        if (debug_variant ? id != named : !((r.algos >> algo) & 1)) continue;
        if (r.domain[dir] && !r.domain[dir](c.dtype, c.p)) continue;
        if (a && !(aligned(ptrs[0], a) && aligned(ptrs[1], a) && aligned(ptrs[2], a))) continue;
        if (a && dir == BWD && r.align_grads && !(aligned(c.g1, a) && aligned(c.g2, a))) continue;
        if (dir == FWD && (c.p.out_bs % r.out_bs_div != 0 || (walk && r.auto_gate && !r.auto_gate(c.p)))) continue;
        if (n < max) ids[n] = id;
        ++n;
    }
    return n ? n : FN2_EUNSUPPORTED;
}

} // namespace

int corr_dispatch(int dir, CorrCall &c, int algo, bool debug_variant, hipStream_t s)
{
    int ids[FN2_CORR_KERNEL_COUNT];
    const int n = corr_plan(dir, c, algo, debug_variant, ids, FN2_CORR_KERNEL_COUNT);
    int rc = n;   // <= 0: nothing to launch
    // only FN2_CORR_AUTO plans more than one kernel: one that declines (task table / index limits; nothing launched) hands over
    for (int i = 0; i < n && (i == 0 || rc == FN2_EUNSUPPORTED || rc == FN2_EALIGN); ++i) {
        // f16x2: its profiling switches.  fp32 MFMA forward: algo itself (0 auto, 2 fp32 MFMA, 3 bf16x3, >= 100 profiling instantiations);
        // backward: 0 = automatic (bf16x3 where its extra preconditions hold), 6 = fp32 MFMA, 4 = bf16x3 or FN2_EUNSUPPORTED, algo - 100
        c.tune = 0;
        if (ids[i] == FN2_CORR_KERNEL_F16X2 && debug_variant) c.tune = algo - (dir == FWD ? 5000 : 6000);
        if (ids[i] == FN2_CORR_KERNEL_MFMA_F32)
            c.tune = dir == FWD ? algo : algo == FN2_CORR_MFMA_F32 ? 6 : algo == FN2_CORR_MFMA_BF16X3 ? 4 : debug_variant ? algo - 100 : 0;
        rc = kCorrRows[ids[i]].launch[dir](c, s);
    }
    return rc;
}

} // namespace fn2

// Every correlation entry point of this file: the argument checks in their order, then the walk -- or, with max_ids >= 0, its plan
static int corr_impl(int dir, fn2::CorrCall c, int B, int C, int H, int W, int pad_size, int kernel_size, int max_displacement, int stride1,
                     int stride2, int64_t out_batch_stride, float negative_slope, int algo, bool debug_variant, void *stream,
                     int *ids = nullptr, int max_ids = -1)
{
    using namespace fn2;
    if (!dtype_size(c.dtype)) return FN2_EDTYPE;
    const int rc = corr_make_params(c.p, B, C, H, W, pad_size, kernel_size, max_displacement, stride1, stride2);
    if (rc != FN2_OK) return rc;
    // the reference's backward indexes (and writes) out of bounds for stride1 != 1
    if (dir == BWD && stride1 != 1) return FN2_EUNSUPPORTED;
    if (dir == FWD && (out_batch_stride < c.p.out_bs || !(negative_slope == negative_slope))) return FN2_EINVAL;
    if (dir == FWD) { c.p.out_bs = out_batch_stride; c.p.slope = negative_slope; }
    if (max_ids >= 0) return corr_plan(dir, c, algo, debug_variant, ids, max_ids);
    return corr_dispatch(dir, c, algo, debug_variant, static_cast<hipStream_t>(stream));
}

extern "C" int fn2_correlation_forward_fused(const void *in1, const void *in2, void *out, int64_t out_batch_stride,
                                             float negative_slope, int dtype, int B, int C, int H, int W,
                                             int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                             int algo, void *stream)
{
    return corr_impl(fn2::FWD, {dtype, {}, in1, in2, nullptr, out, nullptr, nullptr, 0}, B, C, H, W, pad_size, kernel_size,
                     max_displacement, stride1, stride2, out_batch_stride, negative_slope, algo, false, stream);
}

extern "C" int fn2_correlation_forward_ex(const void *in1, const void *in2, void *out, int dtype,
                                          int B, int C, int H, int W,
                                          int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                          int algo, void *stream)
{
    int nOut = 0, oH = 0, oW = 0;
    const int rc = fn2_correlation_output_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2, &nOut,
                                                &oH, &oW);
    if (rc != FN2_OK) return rc;
    return fn2_correlation_forward_fused(in1, in2, out, (int64_t)nOut * oH * oW, 1.0f, dtype, B, C, H, W, pad_size,
                                         kernel_size, max_displacement, stride1, stride2, algo, stream);
}

extern "C" int fn2_correlation_forward(const void *in1, const void *in2, void *out, int dtype,
                                       int B, int C, int H, int W,
                                       int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                       void *stream)
{
    return fn2_correlation_forward_ex(in1, in2, out, dtype, B, C, H, W, pad_size, kernel_size, max_displacement,
                                      stride1, stride2, FN2_CORR_AUTO, stream);
}

extern "C" int fn2_correlation_backward_ex(const void *in1, const void *in2, const void *grad_out,
                                           void *grad_in1, void *grad_in2, int dtype,
                                           int B, int C, int H, int W,
                                           int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                           int algo, void *stream)
{
    return corr_impl(fn2::BWD, {dtype, {}, in1, in2, grad_out, nullptr, grad_in1, grad_in2, 0}, B, C, H, W, pad_size, kernel_size,
                     max_displacement, stride1, stride2, 0, 1.0f, algo, false, stream);
}

extern "C" int fn2_correlation_backward(const void *in1, const void *in2, const void *grad_out,
                                        void *grad_in1, void *grad_in2, int dtype,
                                        int B, int C, int H, int W,
                                        int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                        void *stream)
{
    return fn2_correlation_backward_ex(in1, in2, grad_out, grad_in1, grad_in2, dtype, B, C, H, W, pad_size,
                                       kernel_size, max_displacement, stride1, stride2, FN2_CORR_AUTO, stream);
}

#ifdef FN2_DEBUG_BUILD   // libflownet2_hip_debug.so only (build.py): the product library exports none of this
// ---- profiling / ablation instantiations (fn2_debug.h): not part of the public ABI, outputs may be wrong by design
extern "C" int fn2_debug_correlation_forward(const void *in1, const void *in2, void *out, int dtype, int B, int C, int H, int W,
                                             int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                             int variant, void *stream)
{
    if (variant < 100) return FN2_EINVAL;
    int nOut = 0, oH = 0, oW = 0;
    const int rc = fn2_correlation_output_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2, &nOut, &oH, &oW);
    if (rc != FN2_OK) return rc;
    return corr_impl(fn2::FWD, {dtype, {}, in1, in2, nullptr, out, nullptr, nullptr, 0}, B, C, H, W, pad_size, kernel_size,
                     max_displacement, stride1, stride2, (int64_t)nOut * oH * oW, 1.0f, variant, true, stream);
}

extern "C" int fn2_debug_correlation_backward(const void *in1, const void *in2, const void *grad_out, void *grad_in1,
                                              void *grad_in2, int dtype, int B, int C, int H, int W, int pad_size,
                                              int kernel_size, int max_displacement, int stride1, int stride2, int variant,
                                              void *stream)
{
    if (variant < 100) return FN2_EINVAL;
    return corr_impl(fn2::BWD, {dtype, {}, in1, in2, grad_out, nullptr, grad_in1, grad_in2, 0}, B, C, H, W, pad_size, kernel_size,
                     max_displacement, stride1, stride2, 0, 1.0f, variant, true, stream);
}

extern "C" int fn2_debug_correlation_plan(int direction, const void *in1, const void *in2, void *out, void *grad_in1, void *grad_in2,
                                          int64_t out_batch_stride, int dtype, int B, int C, int H, int W, int pad_size, int kernel_size,
                                          int max_displacement, int stride1, int stride2, int algo, int *ids, int max_ids)
{
    if ((direction != fn2::FWD && direction != fn2::BWD) || max_ids < 0 || (max_ids && !ids)) return FN2_EINVAL;
    int nOut = 0, oH = 0, oW = 0;
    if (direction == fn2::FWD && !out_batch_stride) {   // as fn2_correlation_forward_ex
        const int rc = fn2_correlation_output_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2, &nOut, &oH, &oW);
        if (rc != FN2_OK) return rc;
        out_batch_stride = (int64_t)nOut * oH * oW;
    }
    return corr_impl(direction, {dtype, {}, in1, in2, out, out, grad_in1, grad_in2, 0}, B, C, H, W, pad_size, kernel_size, max_displacement,
                     stride1, stride2, out_batch_stride, 1.0f, algo, algo >= 100, nullptr, ids, max_ids);
}

extern "C" void fn2_debug_set_buffer(void *device_ptr) { fn2::corr_f16x2_set_debug_buffer(device_ptr); }

// Streaming-copy probe (bench.py's `copy_ceiling_GBps`): 16 bytes per lane, grid-stride, four independent loads in flight per
// lane -- the float4 copy MI355X_MICROARCH.md quotes 6.29 TB/s for (read + write bytes).
typedef float scf4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stream_copy_kernel(scf4 *__restrict__ dst, const scf4 *__restrict__ src, size_t n16, int nt)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (nt) {
        for (; i + 3 * stride < n16; i += 4 * stride) {
            const scf4 a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride);
            const scf4 c = __builtin_nontemporal_load(src + i + 2 * stride), d = __builtin_nontemporal_load(src + i + 3 * stride);
            __builtin_nontemporal_store(a, dst + i); __builtin_nontemporal_store(b, dst + i + stride);
            __builtin_nontemporal_store(c, dst + i + 2 * stride); __builtin_nontemporal_store(d, dst + i + 3 * stride);
        }
    } else {
        for (; i + 3 * stride < n16; i += 4 * stride) {
            const scf4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
            dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
        }
    }
    for (; i < n16; i += stride) dst[i] = src[i];
}
// Clock probe (bench.py's `box.mfma_probe_TFLOPs`): every SIMD of the chip runs a register-only stream of independent
// v_mfma_f32_16x16x32_f16 from 4 waves -- no memory, no LDS -- so the achieved rate is (matrix-pipe rate) x (the shader clock this
// box sustains under load): the boxes of the pool differ by 20 % on the whole step, this number says whether it is the clock.
__global__ __launch_bounds__(1024) void mfma_probe_kernel(float *sink, int iters)
{
    typedef float pf4 __attribute__((ext_vector_type(4)));
    typedef _Float16 ph8 __attribute__((ext_vector_type(8)));
    const int lane = threadIdx.x & 63;
    pf4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = (pf4){0.0f, 0.0f, 0.0f, 0.0f};
    ph8 a, b;
#pragma unroll
    for (int i = 0; i < 8; ++i) { a[i] = (_Float16)(0.001f * (lane + i)); b[i] = (_Float16)(0.002f * (lane - i)); }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[i], 0, 0, 0);
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678f) sink[threadIdx.x] = s;
}
// launches the probe; returns the number of MFMA FLOP it executes in *flop (0 on error)
extern "C" int fn2_debug_mfma_probe(void *sink, int iters, int workgroups, double *flop, void *stream)
{
    if (!sink || iters < 1 || workgroups < 1 || !flop) return FN2_EINVAL;
    hipLaunchKernelGGL(mfma_probe_kernel, dim3((unsigned)workgroups), dim3(1024), 0, static_cast<hipStream_t>(stream),
                       static_cast<float *>(sink), iters);
    *flop = (double)workgroups * 16.0 * iters * 8.0 * 16384.0;   // 16 waves x iters x 8 MFMAs x 2 * 16 * 16 * 32 FLOP
    return fn2::launch_status();
}

// Where do the workgroups of a 1-D grid run?  out[b] = HW_REG_XCC_ID of workgroup b.  The kernels' tile orders (xcd_remap) assume
// "workgroup b runs on XCD b % 8" for SPEED only (neighbouring tiles share an L2); bench.py reports the census with its box probes.
__global__ void xcc_census_kernel(int *out)
{
    int x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    if (threadIdx.x == 0) out[blockIdx.x] = x & 15;
}
extern "C" int fn2_debug_xcc_census(int *out, int workgroups, void *stream)
{
    if (!out || workgroups < 1) return FN2_EINVAL;
    hipLaunchKernelGGL(xcc_census_kernel, dim3((unsigned)workgroups), dim3(64), 0, static_cast<hipStream_t>(stream), out);
    return fn2::launch_status();
}

extern "C" int fn2_debug_stream_copy(void *dst, const void *src, size_t bytes, int blocks, int nontemporal, void *stream)
{
    if (!dst || !src || (bytes % 16) || !fn2::aligned(dst, 16) || !fn2::aligned(src, 16) || blocks < 1) return FN2_EINVAL;
    hipLaunchKernelGGL(stream_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<scf4 *>(dst), static_cast<const scf4 *>(src), bytes / 16, nontemporal);
    return fn2::launch_status();
}
#endif
