/*
 * flownet2_hip_sample.h -- C ABI of libflownet2_hip_sample.so: CorrSample, the lookup of a PREBUILT all-pairs correlation
 * pyramid -- RAFT's default `CorrBlock` (`alternate_corr=False`) and that of its descendants (GMA, RAFT-Stereo, CRAFT,
 * SEA-RAFT).  Hand-written gfx950 (MI355X) HIP kernels, a library of its own: it links none of the other libraries and adds
 * nothing to them.  Every name here starts with fn2p_.
 *
 * PREVIEW.  This header lives under include/preview/: the library is built, tested and documented like the released ones, but
 * it is not yet part of their record (include/ *.h).  FN2P_ABI_VERSION is 0: names, signatures and macros may change until the
 * library is released.
 *
 * Conventions are those of flownet2_hip.h: device memory, contiguous; `stream` is a hipStream_t (work is enqueued on it,
 * never synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a
 * rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.
 * Element-type values and return codes are the main header's, restated below under the same names and values (and left out if
 * any of the other headers came first), so a translation unit may include every header of the project, this one last.
 */
#ifndef FLOWNET2_HIP_SAMPLE_H
#define FLOWNET2_HIP_SAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2P_ABI_VERSION 0 /* preview: may change until released */

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H) && !defined(FLOWNET2_HIP_LOOKUP_H) && !defined(FLOWNET2_HIP_UPSAMPLE_H) && \
    !defined(FLOWNET2_HIP_SPLAT_H) && !defined(FLOWNET2_HIP_CENSUS_H) && !defined(FLOWNET2_HIP_SMOOTH_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2p_abi_version(void); /* FN2P_ABI_VERSION */

/*
 * The operation.  float32 throughout.
 *
 *   levels   L of them, 1 <= L <= FN2P_MAX_LEVELS.  Level l is a contiguous tensor (B H W) x H2_l x W2_l -- RAFT's
 *            (B H W, 1, H2_l, W2_l).  Query pixel p = (b H + y) W + x owns SLICE p of every level.  The sizes of the levels are
 *            independent of each other and of H, W; each may be 1.
 *   coords   B x 2 x H x W, channel 0 = x, channel 1 = y, in level-0 cells.
 *   radius   r in 0 .. FN2P_MAX_RADIUS.  D = 2 r + 1, G = 2 r + 2.
 *   out      B x (L D^2) x H x W.
 *
 * Per level l, with c = coords * 2^-l (one fp32 multiply: exact apart from underflow):
 *
 *   x0 = floor(cx), y0 = floor(cy), fx = fl(cx - x0), fy = fl(cy - y0)                     (fp32)
 *   out[b, l D^2 + i D + j, y, x] = ((w00 V(i,j) + w10 V(i+1,j)) + w01 V(i,j+1)) + w11 V(i+1,j+1), summed from +0
 *   V(u,v) = level l's cell (x0 - r + u, y0 - r + v) of slice p: the pixel's GRID point (u,v), 0 <= u,v < G
 *   w00 = (1-fx)(1-fy), w10 = fx (1-fy), w01 = (1-fx) fy, w11 = fx fy
 *
 * Every product and every sum is rounded on its own (multiply and add are two roundings).  The outer window index i moves x,
 * the inner j moves y: the channel order of RAFT's CorrBlock (grid_sample, align_corners, zero padding) and of CorrLookup
 * (flownet2_hip_lookup.h).  fx = fl(cx - x0) is the fp32 difference: it is exact for cx >= 0 and cx <= -1 and rounded once
 * (|error| <= 2^-25) for -1 < cx < 0; the definition, and the float64 reference of the tests, take that fp32 value.
 *
 * Absent terms.  A corner whose cell lies outside the level is ABSENT, not a zero factor; a corner inside is a term even when
 * its weight is 0.  A pixel whose cx or cy (level 0, before the scaling) is not finite or has |c| >= 2^20 has no taps at any
 * level: its L D^2 outputs are +0 and its gradient slices are +0 (the test !(fabsf(c) < 0x1p20f) comes before any float -> int
 * conversion).  The weights are never negative and the sum starts from +0, so adding w * (+0) for an absent cell gives the bits
 * of leaving the term out: the forward kernel stages absent cells as +0 and adds them.
 *
 * Backward.  coords has no gradient.  The gradient of slice p of level l is a gather: for grid point (u,v) inside the level
 *
 *   wg(u,v) = ((gO[u,v] w00 + gO[u-1,v] w10) + gO[u,v-1] w01) + gO[u-1,v-1] w11, summed from +0
 *
 * with gO[i,j] the pixel's grad_out of channel l D^2 + i D + j; terms whose i or j is outside 0 .. D-1 are left out.  Every other
 * cell of the slice is +0.  No two query pixels share memory of a level, so nothing is accumulated: the gradient tensors are
 * FULLY WRITTEN by one kernel, without pre-zeroing, memset node or atomics, and the result is bit-reproducible across runs and
 * streams.  The forward's output is fully written as well.
 *
 * Per-element bounds against a float64 evaluation on the fp32 inputs, u = 2^-24 per rounding.  A term carries at most 7
 * roundings (3 in its weight, 1 product, at most 3 sums); (1+u)^7 - 1 < 2^-21, so
 *   forward   |err| <= 2^FN2P_BOUND_LOG2 S + 8 * 2^-149, S = the element's sum of |w V| over its terms, w the exact product of
 *             the fp32 fx, fy factors;
 *   backward  the same with S = sum |gO w|; exactly 0 where no term arrives.
 * The second summand covers roundings into the fp32 subnormal range.
 *
 * Domain: finite level values and gradients.  Anything else neither faults nor writes outside the outputs; its values are not
 * pinned.
 *
 * Kernels.  One launch per call covers all levels.  Forward: a workgroup of 256 lanes owns FN2P_TILE_FORWARD consecutive pixels
 * of one batch item, stages each pixel's G x G patch of a level in LDS (pixel-major, odd pitch) and writes whole segments of
 * one output channel at a time.  Backward: a workgroup owns FN2P_TILE_BACKWARD consecutive pixels, puts their grid weights in
 * LDS and sweeps their slices with 16-byte stores where the address allows, 4-byte stores at the ends.
 *
 * `levels` / `grad_levels`, `H2`, `W2` are HOST arrays of length num_levels, read during the call; the kernels get their
 * contents by value, so a call captured into a hipGraph replays with the captured pointers and sizes.
 *
 * Checks, all before a launch, in this order:
 *   1. num_levels outside 1 .. FN2P_MAX_LEVELS, radius outside 0 .. FN2P_MAX_RADIUS, B < 0, H < 1, W < 1, or (where the size
 *      arrays are given) a level size < 1: FN2_EINVAL;
 *   2. B H W >= 2^31, or (where the size arrays are given) a slice of 2^31 cells or more, or more than 2^48 cells in a level:
 *      FN2_EUNSUPPORTED (with B H W < 2^31 no grid exceeds the launch limits);
 *   3. B == 0: FN2_OK, nothing launched;
 *   4. a NULL array, a NULL level pointer, NULL coords / out / grad_out: FN2_EINVAL;
 *   5. a pointer not aligned to 4 bytes: FN2_EALIGN.
 * Slice bases are 64-bit: 8 x (55 * 128)^2 cells already pass 2^28.
 */
#define FN2P_MAX_LEVELS 8
#define FN2P_MAX_RADIUS 8
#define FN2P_BOUND_LOG2 -21
#define FN2P_TILE_FORWARD 32
#define FN2P_TILE_BACKWARD 16

int fn2p_corr_sample_forward(const void *const *levels, const int *H2, const int *W2, int num_levels, const void *coords, void *out,
                             int B, int H, int W, int radius, void *stream);
int fn2p_corr_sample_backward(const int *H2, const int *W2, int num_levels, const void *coords, const void *grad_out,
                              void *const *grad_levels, int B, int H, int W, int radius, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_SAMPLE_H */
