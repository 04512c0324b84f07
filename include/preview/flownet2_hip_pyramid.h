/*
 * flownet2_hip_pyramid.h -- C ABI of libflownet2_hip_pyramid.so: CorrPyramid, the BUILD of RAFT's all-pairs correlation pyramid
 * (`CorrBlock.__init__` of `core/corr.py`: matmul, division by sqrt(C), avg_pool2d per further level) in one kernel, and the fold of
 * the levels' gradients back into the gradient of the volume.  Hand-written gfx950 (MI355X) HIP kernels, a library of its own: it
 * links none of the other libraries and adds nothing to them.  Every name here starts with fn2y_ (the lookup of the finished
 * pyramid is fn2p_, include/preview/flownet2_hip_sample.h; the two headers may be included together, this one last).
 *
 * INCUBATING.  This header lives under include/preview/: the library is built, tested and documented like the released ones, but
 * it is not part of their record (include/ *.h) nor of the preview record.  FN2Y_ABI_VERSION is 0: names, signatures and macros may
 * change until the library is released.
 *
 * Conventions are those of flownet2_hip.h: device memory, contiguous; `stream` is a hipStream_t (work is enqueued on it,
 * never synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a
 * rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.
 * Element-type values and return codes are the main header's, restated below under the same names and values (and left out if
 * any of the other headers came first), so a translation unit may include every header of the project, this one last.
 */
#ifndef FLOWNET2_HIP_PYRAMID_H
#define FLOWNET2_HIP_PYRAMID_H

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2Y_ABI_VERSION 0 /* incubating: may change until released */

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H) && !defined(FLOWNET2_HIP_LOOKUP_H) && !defined(FLOWNET2_HIP_UPSAMPLE_H) && \
    !defined(FLOWNET2_HIP_SPLAT_H) && !defined(FLOWNET2_HIP_CENSUS_H) && !defined(FLOWNET2_HIP_SMOOTH_H) && !defined(FLOWNET2_HIP_SAMPLE_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2y_abi_version(void); /* FN2Y_ABI_VERSION */

/*
 * The operation.  float32 throughout.
 *
 *   fmap1    B x C x H x W, fmap2  B x C x H2 x W2.  Query pixel p = (b H + y) W + x owns SLICE p of every level.
 *   levels   L of them, 1 <= L <= FN2Y_MAX_LEVELS.  Level l is a contiguous tensor (B H W) x H2_l x W2_l -- RAFT's
 *            (B H W, 1, H2_l, W2_l) -- with H2_l = H2 >> l, W2_l = W2 >> l: avg_pool2d(2, 2) applied l times, a ragged last row or
 *            column dropped at each step.  A level with H2_l == 0 or W2_l == 0 is refused.
 *
 *   level 0     v0[p, v, u] = fl32( s * sum_c fmap1[b,c,y,x] fmap2[b,c,v,u] ),  s = (float)(1.0 / sqrt((double)C)).
 *               The sum runs on the bf16 matrix cores: each fp32 operand is split exactly into three bf16 terms h + m + l (8 + 8 + 8
 *               significant bits, |m| <= 2^-8 |x|, |l| <= 2^-16 |x|); a product keeps hh, hm, mh, hl, lh, mm and drops ml, lm, ll;
 *               the 6 C partial products are accumulated in fp32, in an order this header does not pin.
 *   level l+1   fl32( ((a + b) + (c + d)) * 0.25f ) of the STORED fp32 values of level l: a, b the top-left and top-right cell of
 *               the 2 x 2 block, c, d the bottom-left and bottom-right.  Every add is rounded on its own, in this order.  Levels
 *               >= 1 are therefore a bit-exact function of level 0 as written.
 *
 * Coverage.  Every element of every level is written exactly once by one kernel: no clear, no atomics, and the same bits on every
 * run and stream.
 *
 * Non-finite inputs.  An output element is non-finite exactly where a float64 evaluation of the composition is; WHICH non-finite
 * value it holds is unspecified (the split turns an inf into NaN terms).  Nothing faults or is written outside the levels.
 *
 * Bound, per element, against a float64 evaluation on the fp32 inputs.  With S0 = s sum_c |fmap1 fmap2| (the element's sum of
 * absolute products, scaled) and U23 = 2^-23:
 *
 *   d0  = FN2Y_BOUND_SPLIT S0 + C FN2Y_BOUND_PER_CHANNEL S0 + U23 |ref| + ((6 C + 1) / C + 1) 2^-149
 *   d_l = pool_l(d0) + l FN2Y_BOUND_PER_POOL pool_l(S0),      pool_l = the exact mean over the 2^l x 2^l block
 *
 * Derivation.  Split: the three dropped cross terms of a product are below (2^-8 2^-16 + 2^-16 2^-8 + 2^-32) |a b| = (2 2^-24 +
 * 2^-32) |a b|: FN2Y_BOUND_SPLIT.  Accumulation: 6 C partial products, each exact in fp32 (8 x 8 bits) and at most (1 + 2^-7)
 * |a b| together per term pair, summed in fp32 in any order: each of the 6 C adds rounds a partial sum no larger than (1 + 2^-7)
 * S0 / s by at most U23 relative (U23, not 2^-24: the matrix core's adder is not assumed to round to nearest): 6 U23 (1 + 2^-7)
 * per channel, FN2Y_BOUND_PER_CHANNEL.  The scale: the reference multiplies by the float64 1 / sqrt(C); fl32 of it and the product
 * are two roundings of 2^-24 each, U23 |ref| (their 2^-48 cross term is far below the slack of the accumulation term).  The
 * last summand is one subnormal step per rounding; it holds for operands in fp32's normal range above 2^-110.  Pooling: a level
 * l + 1 cell is the exact mean of four level-l cells plus three rounded adds (the multiply by 0.25 is exact above the subnormal
 * range); each add rounds a partial sum no larger than 4 pool(S0) (1 + small) by 2^-24 relative, and the sum is then divided by 4:
 * 3 2^-24 pool(S0) per step, stated as 3 U23 = FN2Y_BOUND_PER_POOL with a factor of two to spare.  The error already in the level-l
 * cells averages: pool(d_l).  The bound is this form of tests/corr_contract_ref.py delta_bf16x3 with n = C.  n may be taken as
 * the number of the element's channels whose product is not zero (a zero factor adds exact zeros): C FN2Y_BOUND_PER_CHANNEL
 * becomes n_nz FN2Y_BOUND_PER_CHANNEL, and an element without such a channel is +0 (tests/test_gpu_split_terms.py).
 *
 * Backward.  Given the gradients g_0 .. g_{L-1} of the levels (a missing one counts as zero), the gradient of level 0 as the
 * composition would have accumulated it -- the gradient of the all-pairs volume before the scale is undone -- is the FOLD
 *
 *   G[p,v,u] = fl32( s * (((g0 + 1/4 g1[v>>1,u>>1]) + 1/16 g2[v>>2,u>>2]) + 1/64 g3[v>>3,u>>3]) )
 *
 * where g_l is read at slice p.  A level's term is ABSENT (not a zero summand) where (v >> l) >= H2_l or (u >> l) >= W2_l -- the
 * ragged rows and columns the pooling dropped -- and where the level's pointer is NULL; the sum starts from g0, or from +0 where g0
 * is missing.  The power-of-two products are exact, every add is rounded on its own in this order, then the product with s: G
 * has the bits of a float32 restatement in this order.  G is (B H W) x H2 x W2 and FULLY WRITTEN by one streaming kernel, 16-byte
 * loads and stores on the level-0 rows where W2 % 4 == 0 and the level-0 pointers are 16-byte aligned.  The two contractions that
 * follow,
 *   grad_fmap1[b,c,p] = sum_q G[p,q] fmap2[b,c,q],     grad_fmap2[b,c,q] = sum_p G[p,q] fmap1[b,c,p],
 * are plain batched matrix products and not part of this library.
 *
 * Kernels.  Forward: a workgroup of 256 lanes owns FN2Y_TILE_QUERIES consecutive query pixels of one batch item and an
 * FN2Y_TILE_ROWS x FN2Y_TILE_COLS block of fmap2 aligned to 8 in both directions, so every 2 x 2, 4 x 4 and 8 x 8 pooling block
 * lies inside one tile; per 32 channels both operands are split once into LDS (channels beyond C are zeros), each wave runs
 * v_mfma_f32_32x32x16_bf16 over 32 queries x the whole block, and the epilogue scales the accumulators, stores level 0 and pools
 * levels 1 .. 3 in registers (lane exchanges inside groups of 2, 4 and 8 neighbouring columns).  Lanes cover the contiguous target
 * columns of one query's row.  Slice bases are 64-bit.  The level pointers and sizes travel by value in the kernel arguments, so a
 * call captured into a hipGraph replays with the captured pointers and sizes.
 *
 * `levels` / `grad_levels` are HOST arrays of length num_levels, read during the call.
 *
 * Checks, all before a launch, in this order (both entry points):
 *   1. num_levels outside 1 .. FN2Y_MAX_LEVELS, B < 0, C < 1, H < 1, W < 1, H2 < 1, W2 < 1, or H2 >> (num_levels - 1) == 0 or
 *      W2 >> (num_levels - 1) == 0: FN2_EINVAL;
 *   2. B H W >= 2^31, H2 W2 >= 2^31, more than 2^48 cells in level 0, or C > 2^20: FN2_EUNSUPPORTED;
 *   3. B == 0: FN2_OK, nothing launched;
 *   4. forward: NULL fmap1, fmap2, `levels` or one of its entries; fold: NULL `grad_levels` or G (a NULL ENTRY of grad_levels is a
 *      missing gradient and allowed): FN2_EINVAL;
 *   5. a pointer not aligned to 4 bytes: FN2_EALIGN;
 *   6. forward: B ceil(H W / FN2Y_TILE_QUERIES) ceil(H2 / FN2Y_TILE_ROWS) ceil(W2 / FN2Y_TILE_COLS) >= 2^31 workgroups:
 *      FN2_EUNSUPPORTED.
 */
#define FN2Y_MAX_LEVELS 4
#define FN2Y_TILE_QUERIES 128
#define FN2Y_TILE_ROWS 8
#define FN2Y_TILE_COLS 32
#define FN2Y_BOUND_SPLIT (2 * 0x1p-24 + 0x1p-32)
#define FN2Y_BOUND_PER_CHANNEL (6 * 0x1p-23 * (1 + 0x1p-7))
#define FN2Y_BOUND_PER_POOL (3 * 0x1p-23)

int fn2y_corr_pyramid_forward(const void *fmap1, const void *fmap2, void *const *levels, int num_levels, int B, int C, int H, int W,
                              int H2, int W2, void *stream);
int fn2y_corr_pyramid_fold(const void *const *grad_levels, int num_levels, void *G, int B, int C, int H, int W, int H2, int W2,
                           void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_PYRAMID_H */
