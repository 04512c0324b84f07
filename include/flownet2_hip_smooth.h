/*
 * flownet2_hip_smooth.h -- C ABI of libflownet2_hip_smooth.so: the edge-aware smoothness regulariser of first or second order,
 * the third term of unsupervised optical flow (UnFlow, ARFlow, UFlow, SMURF) next to the census distance and the occlusion
 * estimate.  A robust function of the flow's first or second differences in x and in y, each weighted by exp(-edge measure) of
 * the image difference over the same span; the result is two planes, one per direction.  Hand-written gfx950 (MI355X) HIP
 * kernels, a library of its own: it links none of libflownet2_hip.so, libflownet2_hip_ext.so, libflownet2_hip_lookup.so,
 * libflownet2_hip_upsample.so, libflownet2_hip_splat.so, libflownet2_hip_census.so and adds nothing to them.  Every name here
 * starts with fn2m_.
 *
 * Conventions are those of flownet2_hip.h: NCHW device memory, contiguous; `stream` is a hipStream_t (work is enqueued on it,
 * never synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a
 * rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.
 * Return codes are the main header's, restated below under the same names and values (and left out if one of the other six
 * headers came first), so a translation unit may include all seven headers, this one last.
 */
#ifndef FLOWNET2_HIP_SMOOTH_H
#define FLOWNET2_HIP_SMOOTH_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2M_ABI_VERSION 1

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H) && !defined(FLOWNET2_HIP_LOOKUP_H) && !defined(FLOWNET2_HIP_UPSAMPLE_H) && \
    !defined(FLOWNET2_HIP_SPLAT_H) && !defined(FLOWNET2_HIP_CENSUS_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2m_abi_version(void); /* FN2M_ABI_VERSION */

/*
 * The operation.  flow: N x F x H x W, F = 1 .. 4 (1 for disparity, 2 for flow); image: N x C x H x W, C = 1 or 3; out:
 * N x 2 x H x W, plane 0 the x term, plane 1 the y term; all float32.  Parameters: order k in {1, 2}, edge_weighting
 * FN2M_EDGE_EXPONENTIAL (0) or FN2M_EDGE_GAUSSIAN (1), alpha >= 0 (UFlow's edge constant: 150 for images in [0, 1]) and eps >= 0
 * (UFlow: 0.001; eps = 0 is the plain L1 form).  Every operation below is fp32, rounded on its own, no contraction;
 * csrc/smooth_arith.h holds it, host and device.  For the x direction at pixel (y, x) with x < W - k (the y direction is the same
 * along y, for y < H - k):
 *
 *   image     dI_c = I_c[y, x + k] - I_c[y, x]        t_c = alpha dI_c        a_c = |t_c| (exponential) or t_c t_c (gaussian)
 *   edge      e = ((a_0 + a_1) + a_2) fl32(1 / 3) for C = 3, e = a_0 for C = 1        w = exp2(-(e fl32(log2 e)))      (w = exp(-e))
 *   flow      order 1: d_f = f[y, x + 1] - f[y, x]        order 2: d_f = (f[y, x + 2] - f[y, x + 1]) - (f[y, x + 1] - f[y, x])
 *   robust    eps2 = fl32(eps eps)        rho_f = sqrt(d_f d_f + eps2), and rho_f = |d_f| exactly if eps2 = 0
 *   output    out[n, 0, y, x] = w (((rho_0 + rho_1) + rho_2) + rho_3): ascending f, starting from rho_0
 *   border    exactly +0 where the stencil does not fit: the last k columns of plane 0, the last k rows of plane 1; a plane with
 *             W <= k (or H <= k) is all +0.  Every element of out is written; nothing is pre-zeroed.
 * exp2, sqrt and rsq are the hardware's (each within 1 ulp); exp2(-0) = 1 exactly, so a constant image gives w = 1; a w below
 * 2^-126 is flushed to 0.
 *
 * Backward, flow only (the image gets no gradient), a gather: no atomics, no workspace, bit-reproducible; w and d are recomputed
 * from flow and image.  gO' = grad_out where the stencil fits, +0 elsewhere (a select: a NaN there is harmless).  Per direction,
 * cell and channel
 *   t_f = (gO' w) rho'(d_f)        rho'(d) = d rsq(d d + eps2), and sign(d) (0 at d = 0) exactly if eps2 = 0
 * and for pixel q, with the cells q - j along the direction (t = 0 for a cell outside the image),
 *   order 1: g = t[q - 1] - t[q]        order 2: g = (t[q - 2] - 2 t[q - 1]) + t[q]        grad_flow[n, f, q] = g_x + g_y
 * Outputs are fully written, no pre-zeroing.
 *
 * Domain: finite inputs with |flow| < 2^60; eps = 0 or eps >= 2^-60 (below that fl32(eps eps) loses its bits; if it is 0 the L1
 * form is taken).  Anything else neither faults nor writes outside the outputs; its values are not pinned.
 *
 * Per-element bounds against the float64 evaluation on the fp32 inputs, u = 2^-24.  Per valid cell and flow channel S = 0 for
 * order 1 and S = |f[x + 2] - f[x + 1]| + |f[x + 1] - f[x]| for order 2 (the second difference cancels: its error scales with S):
 *   forward    |err out| <= sum_f [ u ((FN2M_BOUND_A + FN2M_BOUND_E e) w rho + 2 w S) + 2^-126 rho ] + 2^-149 [0 < out < 2^-125]
 *   gradient   |err grad_flow[q]| <= u sum over the taps reaching q of |coef| T,
 *              T = |gO'| (w ((FN2M_BOUND_A + FN2M_BOUND_E e) |rho'| + max(2 S eps^2 / rho^3, 2 D / u)) + 2^-126 / u)
 *                  + 2^-149 / u [0 < |t| < 2^-125]
 *              dd = u |d| (order 1) or u ((1 + u) S + |d|) (order 2), the most the computed d can be off;
 *              eps > 0: D = min(2, dd eps^2 / (max(|d| - dd, 0)^2 + eps^2)^(3/2)), and eps^2 / rho^3 is rho''(d);
 *              eps = 0: D = 2 where |d| <= dd and dd > 0, else 0, and eps^2 / rho^3 = 0
 * with FN2M_BOUND_A = 24 and FN2M_BOUND_E = 16; [c] is 1 where c holds and 0 elsewhere, out and t the exact values; where the
 * bound is 0 the value is exactly 0.  Derivation from the list above:
 *   e        every a_c >= 0, so relative errors add: dI 1 u, t 1 u (gaussian: t t doubles them and adds one: 5 u), the two sums
 *            2 u, the mean 1.5 u (fl32(1/3) is 0.5 u off), the scaling by fl32(log2 e) 1.25 u: below 7 u (exponential) and
 *            10 u (gaussian) of e.  An error delta in exp2's argument is a relative error delta ln 2 in w: below 10 e u.
 *   w        that, and exp2 within 1 ulp (2 u): (2 + 10 e) u.  Below 2^-126 the computed w is 0 and the exact one is less than
 *            2^-126: the 2^-126 terms.
 *   d        order 1: 1 u |d|.  Order 2: the two inner differences are u |f[x+2] - f[x+1]| and u |f[x+1] - f[x]| off, the outer
 *            one rounds what it gets, at most (1 + u) S + |d|: dd.
 *   rho      |rho'| <= 1 and |d| <= rho turn d's error into u (rho + S); d d, eps2 (1.5 u) and the sum are 3.5 u of rho^2, halved
 *            by the root, which adds 2 u: 4.75 u rho + u S.  The sum over f up to 3 u, the product with w 1 u:
 *            forward <= u ((10.75 + 10 e) w rho + w S) per channel, inside 24 + 16 e and 2 S.  A product below 2^-126 is
 *            rounded to a multiple of 2^-149 instead: the last term.
 *   rho'     rho' moves by at most D when d moves by dd.  eps > 0: rho'' = eps^2 / (d^2 + eps^2)^(3/2) decreases in |d|, so over
 *            [|d| - dd, |d| + dd] it is at most its value at max(|d| - dd, 0), and rho' as a whole lies in [-1, 1]: D.  eps = 0:
 *            the computed d has the sign of d wherever |d| > dd; elsewhere rho' is one of {-1, 0, +1}, at most 2 off.  (Up to
 *            ABI 1's first revision this line read "rho'' turns d's error into u (|d| + S) eps^2 / rho^3", the first-order
 *            term at d itself, and 0 for eps = 0.  That holds only while dd is small against max(|d|, eps): on a flow
 *            2^20 x + 0.05 N(0, 1), where u S = 1/8, a correct fp32 evaluation leaves it by 10^5 at eps = 0 and by 10^3 at
 *            eps = 0.001.  The old term stays inside the max, so this bound is nowhere below the old one; on flows of
 *            magnitude 20 the two differ by at most 1.06.)  The sum under rsq 1.75 u, rsq 2 u, the product 1 u, of the computed
 *            |rho'| <= |rho'| + D: 4.75 u |rho'| + (1 + 4.75 u) D.
 *   t        gO' w 1 u, times rho' 1 u: u |gO'| w ((8.75 + 10 e) |rho'| + (1 + 11 u + 10 e u) D / u), inside T as long as
 *            e < 2^20 (beyond that w rounds to 0 in float64 as well); either product, once below 2^-126, is rounded to a
 *            multiple of 2^-149: together the last term.  The gather's five additions at most 5 u of sum |coef| |t|: inside T.
 * These are worst cases; flows and images of ordinary magnitude stay below half of them, typically far below, and the flows that
 * cancel, the graded magnitudes and the flushed weights stay inside them.
 *
 * Kernels: a workgroup of 256 lanes owns FN2M_TILE_H x FN2M_TILE_W output pixels, a wave four rows of it, a lane four vertically
 * adjacent pixels of one column.  The flow and image planes of the tile are staged in LDS, the forward with k rows below and
 * FN2M_HALO_X columns to the right, the backward with k rows above and below and FN2M_HALO_X columns on either side plus the two
 * planes of grad_out, which are turned into gO' w in place before the gather.  Cells outside the image are staged as 0, so the
 * compute phase has no bounds test.  FN2M_HALO_X = 4 >= k keeps every patch row on a 16-byte boundary: where W is a multiple of 4
 * and the tensors are aligned to 16 bytes the tiles are staged with 16-byte loads, otherwise one float at a time.  LDS:
 *   FN2M_LDS_BYTES(planes, k, bwd) = planes * 4 * (FN2M_TILE_H + (bwd ? 2 k : k)) * (FN2M_TILE_W + (bwd ? 2 : 1) * FN2M_HALO_X)
 *   planes = F + C forward, F + C + 2 backward
 * (24480 B forward and 40320 B backward at F = 2, C = 3, k = 2; at most 51840 B).  Every LDS access of the compute phase is a row
 * segment of 64 consecutive floats, conflict-free at any pitch.  No scratch.
 *
 * Checks, all before a launch, in this order: N < 0 or F, C, H or W < 1 (FN2_EINVAL); a plane of 2^31 elements or more, 2^31
 * planes or more or 2^48 elements or more in the widest tensor, or 2^31 workgroups or more (FN2_EUNSUPPORTED); N == 0 (FN2_OK,
 * nothing launched); a NULL tensor pointer (FN2_EINVAL); a pointer not aligned to 4 bytes (FN2_EALIGN); the parameters: C not 1
 * or 3, F above 4, order not 1 or 2, edge_weighting not 0 or 1, alpha or eps not finite or negative (FN2_EINVAL).
 */
#define FN2M_TILE_H 16
#define FN2M_TILE_W 64
#define FN2M_HALO_X 4
#define FN2M_MAX_ORDER 2
#define FN2M_MAX_FLOW_CHANNELS 4
#define FN2M_EDGE_EXPONENTIAL 0
#define FN2M_EDGE_GAUSSIAN 1
#define FN2M_LDS_BYTES(planes, k, bwd) \
    ((planes) * 4 * (FN2M_TILE_H + ((bwd) ? 2 * (k) : (k))) * (FN2M_TILE_W + ((bwd) ? 2 : 1) * FN2M_HALO_X))
#define FN2M_BOUND_A 24
#define FN2M_BOUND_E 16

int fn2m_smoothness_forward(const void *flow, const void *image, void *out, int N, int F, int C, int H, int W, int order,
                            int edge_weighting, float alpha, float eps, void *stream);
int fn2m_smoothness_backward(const void *flow, const void *image, const void *grad_out, void *grad_flow, int N, int F, int C, int H,
                             int W, int order, int edge_weighting, float alpha, float eps, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_SMOOTH_H */
