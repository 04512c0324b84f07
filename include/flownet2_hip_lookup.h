/*
 * flownet2_hip_lookup.h -- C ABI of libflownet2_hip_lookup.so: CorrLookup, the on-demand correlation lookup of RAFT and its
 * descendants (GMA, RAFT-Stereo, CRAFT, SEA-RAFT; RAFT's `alt_cuda_corr`).  Hand-written gfx950 (MI355X) HIP kernels, a library
 * of its own: it links neither libflownet2_hip.so nor libflownet2_hip_ext.so and adds nothing to them.  Every name here starts
 * with fn2l_.
 *
 * Conventions are those of flownet2_hip.h: NCHW device memory, contiguous; `stream` is a hipStream_t (work is enqueued on it,
 * never synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a
 * rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.
 * Element-type values and return codes are the main header's, restated below under the same names and values (and left out if
 * one of the other two headers came first), so a translation unit may include all three headers, this one last.
 */
#ifndef FLOWNET2_HIP_LOOKUP_H
#define FLOWNET2_HIP_LOOKUP_H

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2L_ABI_VERSION 1

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2l_abi_version(void); /* FN2L_ABI_VERSION */

/*
 * The operation.  fmap1: B x C x H x W.  fmap2: B x C x H2 x W2 (any pyramid level: H2, W2 are independent of H, W and may be
 * 1).  coords: B x 2 x H x W, channel 0 = x, channel 1 = y, in fmap2 pixels.  radius r, D = 2 r + 1.  out: B x D^2 x H x W.
 *
 *   x0 = floor(cx), y0 = floor(cy), fx = fl(cx - x0), fy = fl(cy - y0)                     (fp32)
 *   out[b, i D + j, y, x] = scale * sum_{ox,oy in {0,1}} w(ox,oy) * sum_c fmap1[b,c,y,x] * fmap2[b,c, y0 + j - r + oy, x0 + i - r + ox]
 *   w(0,0) = (1-fx)(1-fy), w(1,0) = fx (1-fy), w(0,1) = (1-fx) fy, w(1,1) = fx fy
 *
 * The outer window index i moves x, the inner j moves y: the channel order of RAFT's CorrBlock (grid_sample, align_corners,
 * zero padding, on the all-pairs volume).  fx = fl(cx - x0) is the fp32 difference: it is exact for cx >= 0 and cx <= -1 and
 * rounded once (|error| <= 2^-25) for -1 < cx < 0; the definition, and the float64 reference of the tests, take that fp32 value.
 *
 * Absent terms.  A tap whose integer position lies outside fmap2 is ABSENT, not a zero factor; a tap inside is a term even
 * when its weight is 0.  A pixel whose cx or cy is not finite or has |c| >= 2^20 has no taps: its D^2 outputs are +0, it
 * receives and sends no gradient (the test !(fabsf(c) < 0x1p20f) comes before any float -> int conversion).
 *
 * Gradients.  grad_fmap1[b,c,y,x] = scale sum_k gO[b,k,y,x] * (bilinear sample of fmap2[b,c] at tap k): a gather.
 * grad_fmap2: the transpose, a scatter by float atomic adds (arrival order: not bitwise reproducible from run to run).
 * coords has no gradient.
 *
 * Arithmetic (fp32, multiply and add are two roundings).  The corners of neighbouring taps are the same fmap2 pixels: with
 * G = 2 r + 2 the pixel's GRID point (u,v), 0 <= u,v < G, is fmap2 pixel (x0 - r + u, y0 - r + v).
 *   forward      dots first, then the mix.  g(u,v) = one sequential sum over ascending c, from +0, of fmap1[c] * fmap2[c,grid(u,v)];
 *                out = scale * (((w00 g(i,j) + w10 g(i+1,j)) + w01 g(i,j+1)) + w11 g(i+1,j+1)), from +0, absent corners left out.
 *   grid weight  wg(u,v) = scale * (((gO[u,v] w00 + gO[u-1,v] w10) + gO[u,v-1] w01) + gO[u-1,v-1] w11), from +0, gO[i,j] the
 *                pixel's gradOutput of channel i D + j; terms whose i or j is outside 0 .. D-1 are left out.
 *   grad_fmap1   sum over ascending v, from +0, of (sum over ascending u, from +0, of wg(u,v) * fmap2[c,grid(u,v)]); absent
 *                grid points are left out of both sums.
 *   grad_fmap2   every (pixel, c, grid point inside fmap2) adds wg(u,v) * fmap1[c,y,x] with one float atomic; the output is
 *                cleared on the stream first.
 * The staged kernels walk the channels in chunks of FN2L_CHUNK, which does not change any of these orders.
 *
 * Per-element bounds.  S = |scale| * (the element's sum of |w a b| over its terms: w the exact product of the fp32 fx, fy
 * factors, a, b the two tensor operands; for the gradients a = gO).  A weight carries 3 roundings, the mix / grid weight 5 more
 * (product, 3 adds, scale).  With u = 2^-24 per rounding and (1+u)^n - 1 <= n 2^-24 (1 + 2^-17) for n < 2^7 + C the header's
 * form K 2^-23 S + 2^-23 |exact| has a factor of two in hand:
 *   out         K = FN2L_K_FORWARD(C) = C + 8               (dot: 1 product + C - 1 adds)
 *   grad_fmap1  K = FN2L_K_GRAD1(r)   = 4 r + 13            (8 + product + G - 1 + G adds)
 *   grad_fmap2  |g - exact| <= (n + FN2L_K0_GRAD2) 2^-23 S + 2^-23 |exact| for ANY arrival order, n = the number of terms
 *               (pixel, tap, corner) that reach the element (at least the number of atomic adds), K0 = 10; exactly 0 where no
 *               term arrives.
 * Each bound assumes no intermediate underflow.  A rounding into the fp32 subnormal range adds at most 2^-149 times whatever
 * is multiplied onto it afterwards; where underflow happens only in the products with a tensor operand and their sums (weights
 * <= 1), that is K 2^-149 max(1, |scale|) on top (n + K0 for grad_fmap2), which is what the tests add.
 *
 * Kernels (`algo`):
 *   FN2L_LOOKUP_GENERAL  any valid input, 0 <= r <= FN2L_MAX_RADIUS.  Forward: one lane per (pixel, window row); grad_fmap1:
 *                        one lane per (pixel, channel), grid weights in LDS; every global load is clamped into the tensor.
 *   FN2L_LOOKUP_STAGED   r <= FN2L_STAGED_MAX_RADIUS (otherwise FN2_EUNSUPPORTED, before any launch); forward and grad_fmap1.
 *                        A workgroup owns a tile of FN2L_TILE_W x FN2L_TILE_H pixels, reduces floor(coords) of the tile's
 *                        pixels with taps to a bounding box [xmin, xmax] x [ymin, ymax] and, if
 *                            xmax - xmin + 2 r + 2 <= FN2L_PATCH_W  and  ymax - ymin + 2 r + 2 <= FN2L_PATCH_H,
 *                        stages that fmap2 patch per chunk of FN2L_CHUNK channels in LDS (double-buffered, one barrier per
 *                        step; the forward stages fmap1's tile beside it) and gathers from LDS.  A tile whose box does not
 *                        fit, or without any pixel with taps, runs the general code inside the same kernel.  Every element
 *                        has the BITS of FN2L_LOOKUP_GENERAL.  grad_fmap2 is the atomic scatter under every selector.
 *   FN2L_LOOKUP_AUTO     see the measured points below; both paths give the same bits, so the gate is speed only.
 *   any other value: FN2_EINVAL.
 *
 * AUTO takes the staged kernels (forward and grad_fmap1) for every r <= FN2L_STAGED_MAX_RADIUS and the general ones above; it
 * cannot look at the coordinates before the launch.  Measured on an MI355X (profiles/corr_lookup_micro.json, DESIGN.md 4.11;
 * B = 8, C = 256, r = 4, fp32, general / staged time): coordinates = identity + a smooth flow, maps 48 x 64 and 55 x 128, four
 * pyramid levels each -- forward 1.46 / 2.36 / 1.90 / 1.52 x and 1.82 / 3.05 / 2.73 / 2.06 x (levels 0 .. 3), grad_fmap1
 * 0.90 / 2.43 / 1.79 / 1.21 x and 1.43 / 2.46 / 2.21 / 1.13 x; uniform random coordinates at 48 x 64 (every tile falls back
 * to the general code inside the staged kernel): forward 0.71 x, grad_fmap1 1.00 x -- a caller whose coordinates are scattered
 * selects FN2L_LOOKUP_GENERAL.  Nothing is claimed for other radii, channel counts or flows.
 *
 * Checks, all before a launch, in this order: dtype other than FN2_F32 (FN2_EDTYPE); radius outside 0 .. 8, B < 0, any other
 * size < 1 (FN2_EINVAL); a plane of 2^31 elements or more (FN2_EUNSUPPORTED); B == 0 (FN2_OK, nothing launched); a NULL
 * pointer (FN2_EINVAL); a pointer not aligned to 4 bytes (FN2_EALIGN); the selector (FN2_EINVAL); FN2L_LOOKUP_STAGED with
 * r > FN2L_STAGED_MAX_RADIUS (FN2_EUNSUPPORTED).  Outputs are fully written and need no pre-zeroing: the backward enqueues
 * its own clear of grad_fmap2.
 */
enum { FN2L_LOOKUP_AUTO = 0, FN2L_LOOKUP_GENERAL = 1, FN2L_LOOKUP_STAGED = 2 };

#define FN2L_MAX_RADIUS 8
#define FN2L_STAGED_MAX_RADIUS 4
#define FN2L_TILE_W 16
#define FN2L_TILE_H 4
#define FN2L_PATCH_W 32
#define FN2L_PATCH_H 16
#define FN2L_CHUNK 8
#define FN2L_K_FORWARD(C) ((C) + 8)
#define FN2L_K_GRAD1(r) (4 * (r) + 13)
#define FN2L_K0_GRAD2 10

int fn2l_corr_lookup_forward(const void *fmap1, const void *fmap2, const void *coords, void *out, int dtype, int B, int C, int H,
                             int W, int H2, int W2, int radius, float scale, int algo, void *stream);
int fn2l_corr_lookup_backward(const void *fmap1, const void *fmap2, const void *coords, const void *grad_out, void *grad_fmap1,
                              void *grad_fmap2, int dtype, int B, int C, int H, int W, int H2, int W2, int radius, float scale,
                              int algo, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_LOOKUP_H */
