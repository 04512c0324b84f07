/*
 * flownet2_hip_upsample.h -- C ABI of libflownet2_hip_upsample.so: ConvexUpsample, the learned "convex" upsampling of RAFT and
 * its descendants (`upsample_flow` in RAFT's raft.py) as one fused operation.  Hand-written gfx950 (MI355X) HIP kernels, a
 * library of its own: it links none of libflownet2_hip.so, libflownet2_hip_ext.so, libflownet2_hip_lookup.so and adds nothing to
 * them.  Every name here starts with fn2u_.
 *
 * Conventions are those of flownet2_hip.h: NCHW device memory, contiguous; `stream` is a hipStream_t (work is enqueued on it,
 * never synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a
 * rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.
 * Element-type values and return codes are the main header's, restated below under the same names and values (and left out if
 * one of the other three headers came first), so a translation unit may include all four headers, this one last.
 */
#ifndef FLOWNET2_HIP_UPSAMPLE_H
#define FLOWNET2_HIP_UPSAMPLE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2U_ABI_VERSION 1

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H) && !defined(FLOWNET2_HIP_LOOKUP_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2u_abi_version(void); /* FN2U_ABI_VERSION */

/*
 * The operation.  flow: B x C x H x W, float32, 1 <= C <= FN2U_MAX_CHANNELS.  mask: B x (9 f^2) x H x W, float32, float16 or
 * bfloat16 (`mask_dtype`), the factor f in {2, 4, 8}.  out: B x C x (f H) x (f W), float32.  Mask channel k f^2 + i f + j holds
 * the logit of tap k = 3 ky + kx for sub-row i and sub-column j of the pixel.
 *
 *   m_k  = widen(mask[b, k f^2 + i f + j, y, x])                  k = 0 .. 8   (16-bit values widen exactly)
 *   p_k  = softmax_k(m_k)
 *   v_ck = scale * flow[b, c, y + ky - 1, x + kx - 1]             a tap outside the image is ABSENT from every sum below; its
 *                                                                 p_k stays in the softmax
 *   out[b, c, f y + i, f x + j] = sum_k p_k v_ck
 *
 * which is RAFT's softmax(mask.view(N, 1, 9, f, f, H, W), 2), unfold(f * flow, [3, 3], padding = 1), sum, permute, reshape with
 * scale = f.
 *
 * Gradients.  With gO_c = grad_out[b, c, f y + i, f x + j], d_k = sum_c gO_c v_ck and dbar = sum_k p_k d_k:
 *   grad_mask[b, k f^2 + i f + j, y, x] = p_k (d_k - dbar)        in mask's dtype; an absent tap has d_k = 0, not gradient 0
 *   grad_flow[b, c, y', x'] = scale * sum_k sum_{i,j} p_k(pixel (y' - ky + 1, x' - kx + 1), i, j) * gO_c(that pixel, i, j)
 *                                                                 over the pixels inside the image
 *
 * Input contract: every input finite, scale * flow finite.  Logits of any finite spread: a spread of 1e30 gives weights of
 * exactly 0 and 1.
 *
 * Arithmetic (fp32; multiply and add are two roundings, no contraction; every sum starts from +0, so a sum is never -0).
 *   mx  = max_k m_k;  a_k = m_k - mx;  e_k = expf(a_k);  s = ((e_0 + e_1) + ...) + e_8;  p_k = e_k / s   (IEEE division)
 *   v_ck = scale * flow, rounded; an absent tap takes part as v_ck = +0, which gives the bits of leaving it out
 *   out       = sum over ascending k of p_k * v_ck
 *   d_k       = sum over ascending c of gO_c * v_ck;  dbar = sum over ascending k of p_k * d_k
 *   grad_mask = p_k * (d_k - dbar); for a 16-bit mask that fp32 value rounded to nearest even once -- the 16-bit call has the
 *               bits of the float32 call on the widened mask, rounded once (the forward: the same bits)
 *   T[c,k] of a pixel: its sub-rows are dealt to G = FN2U_GROUPS(f) groups, sub-row i to group i mod G; a group sums p_k * gO_c
 *               over its (i, j) in ascending order; T = ((group 0 + group 1) + ...) in ascending order
 *   grad_flow = scale * (sum over ascending k of T[c,k] of pixel (y' - ky + 1, x' - kx + 1)), pixels outside the image left out
 * No atomics anywhere: both directions are bit-reproducible from run to run and from stream to stream.
 *
 * Per-element bounds against the exact result on the given fp32 / 16-bit values.  u = 2^-24 per rounding; expf is within
 * E = 1 ulp = 2 u relative (HIP documentation, "HIP math API", single precision mathematical functions: expf, maximum error
 * 1 ulp).  a_k carries one rounding, which is a relative error |a_k| u in e_k.  e_k: (2 E + |a_k|) u; s, 8 adds of positive
 * terms: (8 + 2 E + A) u with A = sum_k p_k |a_k|; the division 1: p_k is within pi_k u, pi_k = 4 E + 9 + |a_k| + A.
 *   out        v 1, product 1, 8 adds:  |err| <= 2^-23 sum_k p_k |v_ck| (FN2U_K0_F + |a_k| + A),  K0_F = 4 E + 19 = 23
 *   grad_mask  d_k: (C + 1) <= 5 on D_k = sum_c |gO_c v_ck|; dbar: pi_k' + 5 + 1 + 8 per term; the difference 1, the product 1,
 *              p_k pi_k.  With Sg = sum_k' p_k' D_k':
 *              |err| <= 2^-23 p_k ((D_k + Sg) (FN2U_K0_M + |a_k| + A) + A Sg + sum_k' p_k' D_k' |a_k'|),  K0_M = 8 E + 34 = 42
 *              (the last two terms are dbar's own logit roundings: they belong to the taps k', not to k)
 *              + for a 16-bit mask the output rounding of that fp32 value g: 2^-11 |g| + 2^-25 (float16) or 2^-8 |g| (bfloat16)
 *   grad_flow  product 1, f^2 / G + G - 2 adds in T, 8 in the gather, scale 1:
 *              |err| <= 2^-23 |scale| sum over its terms of p_k |gO| (FN2U_K0_G + |a_k| + A),  K0_G = 4 E + 17 + 64 / 4 + 4 = 41
 *              (counted at f = 8, the largest; f = 4 has 29, f = 2 has 25)
 * The form K 2^-23 against n u has a factor of two in hand, which covers (1 + u)^n - 1 <= n u (1 + 2^-17) and the second order
 * of exp(a_k delta) - 1 for every a_k whose e_k is not 0.  Each bound assumes no intermediate underflow; a rounding into the
 * fp32 subnormal range adds at most 2^-149 times what is multiplied onto it afterwards, for operands up to 1 that is
 * K0 2^-149 max(1, |scale|) on top, which is what the tests add.
 *
 * Kernels.  Forward: a workgroup of FN2U_GROUPS(f) waves owns FN2U_TILE pixels of one row, one lane per pixel; a wave takes the
 * sub-rows of its group, reads the nine mask planes of each sub-position coalesced along x, forms the softmax in registers and
 * turns its f results per channel through LDS into whole output rows, stored as 16 bytes per lane where the row starts on a
 * 16-byte boundary and as single floats where it does not (same values, same bits).  Backward, two kernels and a workspace:
 * the first reads grad_out rows the same way, re-reads the mask once, recomputes the softmax, writes grad_mask and reduces
 * T[b, c, k, y, x] (9 C planes of H x W floats, the workspace); the second gathers grad_flow from T.
 *
 * Checks, all before a launch, in this order: mask_dtype other than FN2_F32, FN2_F16, FN2_BF16 (FN2_EDTYPE); a factor other
 * than 2, 4, 8 (FN2_EINVAL); B < 0 or C, H or W < 1 (FN2_EINVAL); C > FN2U_MAX_CHANNELS, an output plane f H x f W of 2^31
 * elements or more, or 2^31 workgroups or more (FN2_EUNSUPPORTED); B == 0 (FN2_OK, nothing launched); a NULL tensor pointer
 * (FN2_EINVAL); a pointer not aligned to its element size, the workspace to 4 bytes (FN2_EALIGN); in the backward, a NULL
 * workspace (FN2_EINVAL).  Outputs are fully written and need no pre-zeroing; the workspace needs no initialisation and holds
 * nothing the caller needs afterwards.
 */
#define FN2U_MAX_CHANNELS 4
#define FN2U_TILE 64
#define FN2U_GROUPS(f) ((f) < 4 ? (f) : 4)
#define FN2U_K0_F 23
#define FN2U_K0_M 42
#define FN2U_K0_G 41

int fn2u_convex_upsample_forward(const void *flow, const void *mask, void *out, int mask_dtype, int B, int C, int H, int W, int factor,
                                 float scale, void *stream);
/* bytes of `workspace` for these sizes: 9 B C H W floats; 0 for sizes the backward rejects */
size_t fn2u_convex_upsample_backward_workspace_bytes(int B, int C, int H, int W);
int fn2u_convex_upsample_backward(const void *flow, const void *mask, const void *grad_out, void *grad_flow, void *grad_mask,
                                  void *workspace, int mask_dtype, int B, int C, int H, int W, int factor, float scale, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_UPSAMPLE_H */
