/*
 * flownet2_hip_splat.h -- C ABI of libflownet2_hip_splat.so: ForwardWarp, forward flow splatting ("softsplat" summation): every
 * source pixel is moved along its flow and added bilinearly onto the four pixels around where it lands.  The operator behind
 * softmax splatting for frame interpolation, the range-map occlusion estimate of UnFlow / DDFlow / SMURF and forward-projected
 * flow initialisation.  Hand-written gfx950 (MI355X) HIP kernels, a library of its own: it links none of libflownet2_hip.so,
 * libflownet2_hip_ext.so, libflownet2_hip_lookup.so, libflownet2_hip_upsample.so and adds nothing to them.  Every name here
 * starts with fn2s_.
 *
 * Conventions are those of flownet2_hip.h: NCHW device memory, contiguous; `stream` is a hipStream_t (work is enqueued on it,
 * never synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a
 * rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.
 * Return codes are the main header's, restated below under the same names and values (and left out if one of the other four
 * headers came first), so a translation unit may include all five headers, this one last.
 */
#ifndef FLOWNET2_HIP_SPLAT_H
#define FLOWNET2_HIP_SPLAT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2S_ABI_VERSION 1

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H) && !defined(FLOWNET2_HIP_LOOKUP_H) && !defined(FLOWNET2_HIP_UPSAMPLE_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2s_abi_version(void); /* FN2S_ABI_VERSION */

/*
 * The operation.  input: B x C x H x W, float32, any C >= 1.  flow: B x 2 x H x W, float32, channel 0 = x and channel 1 = y (as
 * in Resample2d).  out: B x C x H x W, float32.  fl32() is one rounding to float32, nearest even.  For source pixel (y, x):
 *
 *   fx = fl32(fl32(x) + flow[b,0,y,x])       fy = fl32(fl32(y) + flow[b,1,y,x])       (fl32(x) = x below 2^24)
 *   valid = (fx > -1) && (fx < fl32(W)) && (fy > -1) && (fy < fl32(H))     NaN fails it; tested on the floats, before any
 *                                                                           conversion to an integer
 *   x0 = floor(fx)   y0 = floor(fy)   ax = fl32(fx - x0)   ay = fl32(fy - y0)   bx = fl32(1 - ax)   by = fl32(1 - ay)
 *   w00 = fl32(bx by)   w01 = fl32(ax by)   w10 = fl32(bx ay)   w11 = fl32(ax ay)            (tap dy dx)
 *   out[b, c, y0 + dy, x0 + dx] += fl32(w_dydx * input[b,c,y,x])      for every tap inside the image
 *
 * An invalid pixel contributes nothing and gets zero gradients.  A tap of weight exactly 0 may be skipped (the general kernel
 * skips it; the tiled kernel adds its +-0 to an LDS cell, which changes no bit of the result).  out starts from +0: the entry
 * point clears it on the stream itself, callers need no pre-zeroing.  This tap computation is csrc/splat_taps.h, host and device.
 *
 * Input contract: input finite.  flow may hold anything, NaN, +-inf and +-1e30 included.
 *
 * Gradients, both gathers: no atomics, bit-reproducible.  gO_dydx = grad_out[b, c, y0 + dy, x0 + dx], +0 for a tap outside the
 * image; for an invalid pixel every weight, ax, ay, bx, by and every gO are +0.  Every sum starts from +0, one rounding per
 * operation, no contraction:
 *   grad_input[b,c,y,x] = (((0 + w00 gO00) + w01 gO01) + w10 gO10) + w11 gO11                      tap order 00, 01, 10, 11
 *   grad_flow[b,0,y,x]  = sum over ascending c of input[b,c,y,x] * (by (gO01 - gO00) + ay (gO11 - gO10))
 *   grad_flow[b,1,y,x]  = sum over ascending c of input[b,c,y,x] * (bx (gO10 - gO00) + ax (gO11 - gO01))
 * One lane owns a pixel and walks its channels: nothing is split across lanes or waves.
 *
 * Per-element bounds against the exact result on the given fp32 values of fx, fy, ax, ay, bx, by; u = 2^-24 per rounding, a
 * count of K roundings is written K 2^-23 (a factor of two in hand, which covers (1 + u)^K - 1 and then some):
 *   out         a cell with n contributions: two roundings in w beyond ax, one in the product, n - 1 adds in any order:
 *               |err| <= (n + 2) 2^-23 sum |w v| + (n + 2) 2^-149
 *   grad_input  w 2, product 1, three adds that round (the first adds to +0): FN2S_K_I = 6
 *               |err| <= FN2S_K_I 2^-23 sum_t |w_t gO_t| + FN2S_K_I 2^-149
 *   grad_flow   per channel: difference 1, product 1, sum 1, product with the input 1; C - 1 adds that round: C + FN2S_K_F,
 *               FN2S_K_F = 4 (the C adds counted in full)
 *               |err| <= (C + FN2S_K_F) 2^-23 sum_c |input_c| (by (|gO01| + |gO00|) + ay (|gO11| + |gO10|)) + (C + FN2S_K_F) 2^-149
 *               and likewise for y with bx, ax and the pairs (10, 00), (11, 01)
 * The 2^-149 terms stand for roundings into the subnormal range, for operands up to 1 in magnitude.
 * Results below 2^-126: the fp32 atomic adds of both kernels and the LDS adds of the tiled one keep subnormal sums on gfx950
 * (measured: planes whose every value, and so every sum, is subnormal stay inside the bound above under FN2S_GENERAL, FN2S_TILED
 * and FN2S_AUTO, where a sum flushed to 0 would miss its (n + 2) 2^-149 by a factor of 10^6), so the floor holds
 * as written over the whole domain.  The deterministic forward keeps its bits there too: plane maxima from 2^-127 to 2^126.
 *
 * Kernels (`algo` of fn2s_forward_warp_forward):
 *   FN2S_GENERAL  one lane per source pixel, lanes along x, a loop over channels, one float atomic add per tap inside the
 *                 image.  A flow that is the same for neighbouring pixels gives atomic wave-instructions of contiguous bytes;
 *                 sub-pixel noise already breaks them up.  Correct for every flow.
 *   FN2S_TILED    a workgroup owns FN2S_TILE_H x FN2S_TILE_W source pixels.  It sums their contributions in an LDS patch of
 *                 (FN2S_TILE_H + 2 FN2S_HALO) x (FN2S_TILE_W + 2 FN2S_HALO) cells per channel, FN2S_CHANNEL_GROUP channels at a
 *                 time, with LDS float adds into fp64 cells (the fp32 contribution widened exactly; a cell is rounded to fp32
 *                 once, when it is flushed, so its error is below the bound's).  The patch's origin is the tile's origin -
 *                 FN2S_HALO + (rint(flow x), rint(flow y)) of the tile's centre pixel (clamped into the image; a flow that is
 *                 not a number below 10^6 in magnitude counts as 0).  A workgroup takes a tile and a run of channel groups.
 *                 Each patch row is then added to out with one atomic per non-zero cell, consecutive lanes on
 *                 consecutive cells.  A pixel whose four taps do not all lie in the patch adds straight to out as the general
 *                 kernel does: correct for every flow, only the speed depends on its smoothness.  The order of the additions
 *                 differs from the general kernel's; where every cell has at most one non-zero term both give the same bits.
 *   FN2S_AUTO     see the measured points in DESIGN.md 4.13.
 * Float atomic sums depend on the order of arrival: the forward under these selectors may differ in the last bits from run to
 * run, within the bound above.
 *
 * The deterministic forward, fn2s_forward_warp_forward_det.  Per plane (b, c): M = max |input|, E = frexp exponent of M
 * (2^(E-1) <= M < 2^E), K = ceil(log2(H W)), s = 62 - E - K.  Every contribution v (the fp32 value the atomic path adds) becomes
 * q = rne(v 2^s) as an int64, so |sum q| <= 2^62; the int64 sums are exact and order-free; out = (float)((double)Q 2^-s), both
 * conversions to nearest even.  An all-zero plane gives +0 everywhere.  A plane whose maximum is inf or NaN breaks the input
 * contract and is filled with NaN; other planes are unaffected.  The result is the same bits from run to run, from stream to
 * stream and for every order of arrival; it lies within the bound above plus half a unit of 2^-s per contribution, which is
 * at most 2^(K-62) M per contribution.  Workspace: B C plane maxima (4 bytes each, rounded up to 256 bytes) and B C H W int64
 * cells; the entry point clears it on the stream, it needs no initialisation and holds nothing the caller needs afterwards.
 * out is fully written.  Kernels: plane maxima, the general kernel's shape with 64-bit integer atomics, a conversion pass.
 *
 * Backward: one kernel, one lane per source pixel, a loop over channels; either gradient pointer may be NULL (not wanted; both
 * NULL is FN2_EINVAL).  No workspace.  Outputs fully written, no pre-zeroing.
 *
 * Checks, all before a launch, in this order: B < 0 or C, H or W < 1 (FN2_EINVAL); a plane of 2^31 elements or more, 2^31
 * planes or more, 2^48 elements or more in all, or 2^31 workgroups or more (FN2_EUNSUPPORTED); B == 0 (FN2_OK, nothing
 * launched); a NULL tensor pointer, in the backward both gradients NULL, in the deterministic forward a NULL workspace
 * (FN2_EINVAL); a pointer not aligned to 4 bytes, the workspace to 8 (FN2_EALIGN); a workspace smaller than
 * fn2s_forward_warp_forward_det_workspace_bytes (FN2_EINVAL); the selector (FN2_EINVAL).
 */
#define FN2S_TILE_H 16
#define FN2S_TILE_W 64
#define FN2S_HALO 4
#define FN2S_CHANNEL_GROUP 2
#define FN2S_K_I 6
#define FN2S_K_F 4

enum { FN2S_AUTO = 0, FN2S_GENERAL = 1, FN2S_TILED = 2 };

int fn2s_forward_warp_forward(const void *input, const void *flow, void *out, int B, int C, int H, int W, int algo, void *stream);
/* bytes of `workspace` for these sizes; 0 for sizes the deterministic forward rejects, and for B == 0 */
size_t fn2s_forward_warp_forward_det_workspace_bytes(int B, int C, int H, int W);
int fn2s_forward_warp_forward_det(const void *input, const void *flow, void *out, void *workspace, size_t workspace_bytes, int B, int C,
                                  int H, int W, void *stream);
int fn2s_forward_warp_backward(const void *input, const void *flow, const void *grad_out, void *grad_input, void *grad_flow, int B,
                               int C, int H, int W, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_SPLAT_H */
