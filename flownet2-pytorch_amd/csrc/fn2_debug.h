// fn2_debug.h -- profiling / ablation entry points of libflownet2_hip.so.  NOT part of the public C ABI
// (include/flownet2_hip.h): the instantiations they select skip MFMAs, loads or stores, or dump timestamps into the
// output, so their results are wrong by design.  Used by scripts/ (micro-benchmarks) and a few parity tests of
// alternative tilings.
//   forward variants : 100 .. 4999  instantiations of correlation_mfma.hip (see corr_forward_mfma_f32)
//                      5000 + v     correlation_f16x2.hip with profiling switches v (1 no MFMA, 2 no global loads,
//                                   4 no stores, 8 no operand reads, 16 no split / LDS staging writes)
//   backward variants: 100 + v      instantiations of correlation_mfma_bwd.hip
//   both             : 9000         FN2_DEBUG_CORR_DENSE: the dense stride-1 kernels of correlation_dense.hip by name (kernel_size 1,
//                                   stride1 = stride2 = 1, pad_size == max_displacement in 1 .. 4, float / half / bfloat16), or
//                                   FN2_EUNSUPPORTED outside that domain, decided before anything is launched.  Unlike every other
//                                   variant its results are correct: the bits of FN2_CORR_DIRECT, which is what FN2_CORR_AUTO runs
//                                   there -- this value only makes the choice explicit for tests and benchmarks
#pragma once
#include <stddef.h>
#include <stdint.h>

#define FN2_DEBUG_CORR_DENSE 9000

/* rows of the correlation dispatcher's kernel table (capi.hip), in the order FN2_CORR_AUTO tries them: half / bfloat16 tensors
 * (correlation_f16_*.hip), float with the f16 split (correlation_f16x2*.hip), float on the fp32 / bf16x3 matrix kernels
 * (correlation_mfma*.hip), double (correlation_mfma_f64.hip), dense stride-1 volumes (correlation_dense.hip), the general kernel */
enum { FN2_CORR_KERNEL_H16, FN2_CORR_KERNEL_F16X2, FN2_CORR_KERNEL_MFMA_F32, FN2_CORR_KERNEL_F64, FN2_CORR_KERNEL_DENSE,
       FN2_CORR_KERNEL_DIRECT, FN2_CORR_KERNEL_COUNT };

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)   /* the libraries are built with -fvisibility=hidden */
int fn2_debug_correlation_forward(const void *in1, const void *in2, void *out, int dtype, int B, int C, int H, int W,
                                  int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                  int variant, void *stream);
int fn2_debug_correlation_backward(const void *in1, const void *in2, const void *grad_out, void *grad_in1, void *grad_in2,
                                   int dtype, int B, int C, int H, int W, int pad_size, int kernel_size,
                                   int max_displacement, int stride1, int stride2, int variant, void *stream);
/* What would this call run?  Nothing is launched and no pointer dereferenced (a host test may pass 0x1000).  direction 0:
 * fn2_correlation_forward_fused(in1, in2, out, out_batch_stride, slope 1, ..., algo), with out_batch_stride 0 fn2_correlation_forward_ex;
 * direction 1: fn2_correlation_backward_ex(in1, in2, grad_out = out, grad_in1, grad_in2, ..., algo); algo >= 100: that variant of the two
 * entry points above.  Returns how many FN2_CORR_KERNEL_* the dispatcher would try, the first max_ids of them in ids[] in its order (a
 * launcher that declines hands over to the next), or the negative code the entry point returns before any launch. */
int fn2_debug_correlation_plan(int direction, const void *in1, const void *in2, void *out, void *grad_in1, void *grad_in2,
                               int64_t out_batch_stride, int dtype, int B, int C, int H, int W, int pad_size, int kernel_size,
                               int max_displacement, int stride1, int stride2, int algo, int *ids, int max_ids);
/* resample2d with profiling switches in `flags` (bit 8: untiled kernels, bits 9-11: backward ablations, bits 12-13: tile
 * height 1 = 48, 2 = 32, 3 = 64 rows); the public entry points only look at bilinear != 0 */
int fn2_debug_resample2d_forward(const float *img, const int64_t *img_strides, const float *flow, float *out,
                                 int B, int C, int Hi, int Wi, int H, int W, int kernel_size, int bilinear, int flags, void *stream);
int fn2_debug_resample2d_backward(const float *img, const int64_t *img_strides, const float *flow, const float *grad_out,
                                  float *grad_img, float *grad_flow, int B, int C, int Hi, int Wi, int H, int W,
                                  int kernel_size, int bilinear, int flags, void *stream);
/* device buffer (>= 64 KB) that forward variant 5064 dumps its s_memtime stamps into; NULL = none */
void fn2_debug_set_buffer(void *device_ptr);
/* float4 grid-stride device-to-device copy of `bytes` (multiple of 16) with `blocks` workgroups of 256 lanes: the streaming
 * ceiling bench.py reports next to the 8 TB/s spec peak */
int fn2_debug_stream_copy(void *dst, const void *src, size_t bytes, int blocks, int nontemporal, void *stream);
/* register-only f16 MFMA stream on every SIMD (`workgroups` x 16 waves x iters x 8 MFMAs): a probe of the shader clock the box
 * sustains; *flop receives the FLOP count, `sink` is a device buffer of >= 4 KB that is never written */
int fn2_debug_mfma_probe(void *sink, int iters, int workgroups, double *flop, void *stream);
/* out[b] = HW_REG_XCC_ID of workgroup b of a 1-D grid of `workgroups` (device array of ints) */
int fn2_debug_xcc_census(int *out, int workgroups, void *stream);
#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
