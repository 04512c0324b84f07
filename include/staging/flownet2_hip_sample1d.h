/*
 * flownet2_hip_sample1d.h -- C ABI of libflownet2_hip_sample1d.so (staging): CorrSample1d, the lookup of a PREBUILT 1-D
 * correlation pyramid -- RAFT-Stereo's default `CorrBlock1D` (its `reg` implementation) and that of the stereo networks built
 * on it (IGEV-Stereo, CREStereo's 1-D search).  Hand-written gfx950 (MI355X) HIP kernels, a library of its own: it links none
 * of the other libraries and adds nothing to them.  Every name here starts with fn2h_.  Staging: ABI version 0, may change
 * until the library is released.
 *
 * Conventions are those of flownet2_hip.h: device memory; `stream` is a hipStream_t (work is enqueued on it, never
 * synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a rejected
 * call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.  Return codes are
 * the main header's, restated below under the same names and values (and left out if one of the released, preview or staging
 * headers came first), so a translation unit may include this header alone or after any of them.
 */
#ifndef FLOWNET2_HIP_SAMPLE1D_H
#define FLOWNET2_HIP_SAMPLE1D_H

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2H_ABI_VERSION 0

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H) && !defined(FLOWNET2_HIP_LOOKUP_H) && !defined(FLOWNET2_HIP_UPSAMPLE_H) && \
    !defined(FLOWNET2_HIP_SPLAT_H) && !defined(FLOWNET2_HIP_CENSUS_H) && !defined(FLOWNET2_HIP_SMOOTH_H) &&                            \
    !defined(FLOWNET2_HIP_SAMPLE_H) && !defined(FLOWNET2_HIP_PYRAMID_H) && !defined(FLOWNET2_HIP_SSIM_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2h_abi_version(void); /* FN2H_ABI_VERSION */

/*
 * The operation.  float32 throughout.
 *
 *   levels    L of them, 1 <= L <= FN2H_MAX_LEVELS.  Level l is a contiguous array (B H W) x W2_l -- RAFT-Stereo's
 *             (B H W1, 1, 1, W2_l).  Query pixel p = (b H + y) W + x owns SLICE p of every level.  The sizes of the levels are
 *             independent of each other and of W; each may be 1.
 *   coords_x  one float per query pixel, in level-0 cells, addressed as coords_x[b batch_stride + y W + x] with batch_stride >=
 *             H W in elements: channel 0 of RAFT-Stereo's B x 2 x H x W coordinate tensor is read in place (batch_stride =
 *             2 H W), a B x 1 x H x W tensor as well (H W).  No y channel is ever read.
 *   radius    r in 0 .. FN2H_MAX_RADIUS.  D = 2 r + 1, G = 2 r + 2.
 *   out       B x (L D) x H x W, contiguous.  Channel l D + i is level l, offset i - r: RAFT-Stereo's channel order.
 *
 * Per level l, with c = coords_x * 2^-l (one fp32 multiply: exact apart from underflow):
 *
 *   x0 = floor(c), fx = fl(c - x0), w0 = fl(1 - fx), w1 = fx                                 (fp32)
 *   out[b, l D + i, y, x] = fl( fl(w0 V(i)) + fl(w1 V(i+1)) ), summed from +0
 *   V(u) = cell x0 - r + u of slice p of level l: the pixel's GRID point u, 0 <= u < G
 *
 * Every product and every sum is rounded on its own (multiply and add are two roundings).  fx = fl(c - x0) is the fp32
 * difference: exact for c >= 0 and c <= -1 and rounded once for -1 < c < 0; the definition, and the float64 reference of the
 * tests, take that fp32 value, and w0 = fl(1 - fx) is the fp32 difference as well.  This is grid_sample (bilinear, align_corners,
 * zero padding) on a one-row image, which RAFT-Stereo's bilinear_sampler applies to each level.
 *
 * Absent terms.  A cell outside the level is ABSENT, not a zero factor; a cell inside is a term even when its weight is 0.  A
 * pixel whose coords_x (level 0, before the scaling) is not finite or has |c| >= 2^20 has no taps at any level: its L D outputs
 * are +0 and its gradient slices are +0 (the test !(fabsf(c) < 0x1p20f) comes before any float -> int conversion).  The weights
 * are never negative and the sum starts from +0, so adding w * (+0) for an absent cell gives the bits of leaving the term out:
 * the forward kernel stages absent cells as +0 and adds them.
 *
 * Backward.  coords_x has no gradient.  The gradient of slice p of level l is a gather: for grid point u inside the level
 *
 *   wg(u) = fl( fl(gO[u] w0) + fl(gO[u-1] w1) ), summed from +0
 *
 * with gO[i] the pixel's grad_out of channel l D + i; a term whose i is outside 0 .. D-1 is left out.  Every other cell of the
 * slice is +0.  No two query pixels share memory of a level, so nothing is accumulated: the gradient levels are FULLY WRITTEN by
 * one kernel, without pre-zeroing, memset node or atomics, and the result is bit-reproducible across runs and streams.  The
 * forward's output is fully written by one kernel as well.
 *
 * Per-element bounds against a float64 evaluation on the fp32 inputs, u = 2^-24 per rounding.  A term carries at most 3
 * roundings (1 - fx, the product, the sum); (1+u)^3 - 1 < 2^-22, so
 *   forward   |err| <= 2^FN2H_BOUND_LOG2 S + 4 * 2^-149, S = the element's sum of |w V| over its terms, w the exact value from
 *             the fp32 fx (1 - fx in exact arithmetic, or fx);
 *   backward  the same with S = sum |gO w|; exactly 0 where no term arrives.
 * The second summand covers roundings into the fp32 subnormal range.
 *
 * Domain: finite level values and gradients.  Anything else neither faults nor writes outside the outputs; its values are not
 * pinned.
 *
 * Kernels.  One launch per call covers all levels.  Forward: a workgroup of 256 lanes owns a tile of consecutive pixels
 * of one batch item and stages their G-cell windows of every level in LDS at once (consecutive lanes read consecutive cells of
 * one window; odd pitch), then every lane mixes two cells per output and a wave stores runs of consecutive pixels of one output
 * channel.  Backward: a workgroup owns a tile of consecutive pixels, puts their grid weights wg of every level in LDS
 * and sweeps the ONE contiguous span its pixels own in each gradient level flat, four cells per lane: 16-byte stores where the
 * address allows, 4-byte stores at the span's ends.
 *
 * `levels` / `grad_levels` and `W2` are HOST arrays of length num_levels, read during the call; the kernels get their contents
 * by value, so a call captured into a hipGraph replays with the captured pointers and sizes.
 *
 * Checks, all before a launch, in this order:
 *   1. num_levels outside 1 .. FN2H_MAX_LEVELS, radius outside 0 .. FN2H_MAX_RADIUS, B < 0, H < 1, W < 1, coords_batch_stride
 *      < H W, or (where W2 is given) a level width < 1: FN2_EINVAL;
 *   2. B H W >= 2^31, or (where W2 is given) more than 2^48 cells in a level: FN2_EUNSUPPORTED (a level width is an int: it
 *      cannot reach 2^31; with B H W < 2^31 no grid exceeds the launch limits);
 *   3. B == 0: FN2_OK, nothing launched;
 *   4. a NULL array, a NULL level pointer, NULL coords_x / out / grad_out: FN2_EINVAL;
 *   5. a pointer not aligned to 4 bytes: FN2_EALIGN.
 * Slice bases are 64-bit: 8 x 94 x 311 pixels x 311 cells already pass 2^26, and nothing ties W2 to W.
 */
#define FN2H_MAX_LEVELS 8
#define FN2H_MAX_RADIUS 8
#define FN2H_BOUND_LOG2 -22

int fn2h_corr_sample1d_forward(const void *const *levels, const int *W2, int num_levels, const void *coords_x,
                               long long coords_batch_stride, void *out, int B, int H, int W, int radius, void *stream);
int fn2h_corr_sample1d_backward(const int *W2, int num_levels, const void *coords_x, long long coords_batch_stride,
                                const void *grad_out, void *const *grad_levels, int B, int H, int W, int radius, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_SAMPLE1D_H */
