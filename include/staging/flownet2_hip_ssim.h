/*
 * flownet2_hip_ssim.h -- C ABI of libflownet2_hip_ssim.so (staging): the structural-similarity distance, the photometric term
 * of unsupervised optical flow (ARFlow, UFlow) and of unsupervised stereo / depth (monodepth: 0.85 SSIM + 0.15 L1), next to the
 * census distance.  Hand-written gfx950 (MI355X) HIP kernels, a library of its own: it links none of the other libraries and adds
 * nothing to them.  Every name here starts with fn2i_.  Staging: ABI version 0, may change until the library is released.
 *
 * Conventions are those of flownet2_hip.h: NCHW device memory, contiguous; `stream` is a hipStream_t (work is enqueued on it,
 * never synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a
 * rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.
 * Return codes are the main header's, restated below under the same names and values (and left out if one of the released or
 * preview headers came first), so a translation unit may include this header alone or after any of them.
 */
#ifndef FLOWNET2_HIP_SSIM_H
#define FLOWNET2_HIP_SSIM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2I_ABI_VERSION 0

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H) && !defined(FLOWNET2_HIP_LOOKUP_H) && !defined(FLOWNET2_HIP_UPSAMPLE_H) && \
    !defined(FLOWNET2_HIP_SPLAT_H) && !defined(FLOWNET2_HIP_CENSUS_H) && !defined(FLOWNET2_HIP_SMOOTH_H) &&                            \
    !defined(FLOWNET2_HIP_SAMPLE_H) && !defined(FLOWNET2_HIP_PYRAMID_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2i_abi_version(void); /* FN2I_ABI_VERSION */

/*
 * The operation.  im1 (x), im2 (y), out, grad_out, grad1, grad2: N x C x H x W, float32, any C >= 1; the N C planes are
 * independent.  Parameters: md in {1, 2, 3} (k = 2 md + 1, n = k k), c1 > 0 and c2 > 0 finite (0.01^2 and 0.03^2 for images in
 * [0, 1]), border FN2I_BORDER_ZERO (0) or FN2I_BORDER_REFLECT (1).  Over the k x k window centred at p:
 *
 *   mx = mean x      my = mean y      sx = mean (x - mx)^2      sy = mean (y - my)^2      sxy = mean (x - mx)(y - my)
 *   A1 = 2 mx my + c1      A2 = 2 sxy + c2      B1 = mx^2 + my^2 + c1      B2 = sx + sy + c2
 *   S = A1 A2 / (B1 B2)        out[p] = clamp((1 - S) / 2, 0, 1)
 *
 *   border zero      (ARFlow's SSIM, its valid-only result embedded) the windows that fit: md <= y < H - md, md <= x < W - md.
 *                    Every other element of out -- the ring of width md, or all of a plane with H < k or W < k -- is exactly +0
 *                    and sends no gradient.
 *   border reflect   (monodepth2's SSIM module) both images are extended by md on every side by reflection about the border
 *                    pixel (position -i reads i, position H - 1 + i reads H - 1 - i), then the same windows: every pixel has
 *                    a value.  Needs H > md and W > md.
 * Every element of out is written; nothing is pre-zeroed.
 *
 * Arithmetic, fp32, every operation rounded on its own, no contraction; window cells in row-major order (rows ascending, columns
 * ascending inside a row), starting from the first cell; r = fl32(1 / n):
 *   mx = (x_0 + x_1 + ... ) r                                    (my alike)
 *   sx = ((x_0 - mx)(x_0 - mx) + (x_1 - mx)(x_1 - mx) + ...) r     (sy alike; sxy with the products (x_i - mx)(y_i - my))
 *   A1 = (2 mx) my + c1     A2 = 2 sxy + c2     B1 = (mx mx + my my) + c1     B2 = (sx + sy) + c2
 *   S = (A1 A2) / (B1 B2)   (IEEE division)     d = (1 - S) 0.5     out = min(max(d, 0), 1)
 * The second moments are taken about the computed mean, not as mean x^2 - mx^2: sum (x_i - m)^2 = n sx + n (m - mx)^2 exactly,
 * so an error of the mean enters them at second order and their error is relative to sx itself, however small sx is against
 * x^2 or c2.  For im2 == im1 (the same values) A1 == B1 and A2 == B2 bit for bit, S = 1 and out = +0 exactly.
 *
 * Backward, both images, a gather: no atomics, no workspace, nothing cleared, bit-reproducible.  The statistics are recomputed
 * from im1 and im2 (the same expressions, the same bits as the forward).  Per valid window p, with E = 1 / (B1 B2):
 *   pass = 0 <= d <= 1 (d before the clamp, ends included: torch's clamp)      g' = -0.5 grad_out[p] where pass, else +0 (a select)
 *   Dsxy = (2 A1) E        Ds = -(S / B2)        Dmx = ((2 my) A2) E - ((2 mx) S) / B1        Dmy = ((2 mx) A2) E - ((2 my) S) / B1
 *   gn = g' r       Mx = gn Dmx       My = gn Dmy       A = gn (2 Ds)       B = gn Dsxy
 * and for a position q of the (extended) image, over the windows p that contain it, in row-major order of p,
 *   Gx(q) = sum_p ((Mx_p + A_p (x_q - mx_p)) + B_p (y_q - my_p))        Gy(q) = sum_p ((My_p + A_p (y_q - my_p)) + B_p (x_q - mx_p))
 * (the derivative of S through mx, sx and sxy, with the terms in x_q and in mx_p taken together: each tap is small where the
 * window is flat, nothing cancels across taps).  Border zero: grad1 = Gx, grad2 = Gy; a pixel no valid window contains gets
 * exactly +0.  Border reflect: the gradient is the adjoint of the extension, grad1[q] = sum of Gx over the extended positions that
 * read q -- q itself, -q where 1 <= q <= md, 2 (H - 1) - q where 1 <= H - 1 - q <= md, per axis; x and y have the value of q at all
 * of them, so the kernel gives every tap the integer weight w = wy wx, the number of those positions inside window p, and
 * accumulates w tap.  grad1 or grad2 may be NULL: that gradient is not computed; the other has the same bits.  Outputs are fully
 * written.
 *
 * Domain: finite inputs with |x|, |y| < 2^30, c1 and c2 in [2^-60, 2^60].  Anything else neither faults nor writes outside the
 * outputs; its values are not pinned.
 *
 * Per-element bounds against the float64 evaluation on the fp32 inputs, u = 2^-24, N1 = n + 1, N4 = n + 4 (FN2I_BOUND_MEAN and
 * FN2I_BOUND_MOMENT add to n), X = mean |x| and Y = mean |y| over the window, all quantities exact:
 *   dmx = N1 u X            (dmy alike)        the n - 1 additions of the sum, fl32(1 / n) (u / 2) and the product
 *   esx = N4 u sx + 2 dmx^2 (esy alike)        per term: the difference u, the square 2 u + u; n - 1 additions; r and the product
 *                                              1.5 u; all terms >= 0 so relative errors add; n (m - mx)^2 / n <= dmx^2, doubled
 *   esxy = N4 u sqrt((sx + dmx^2)(sy + dmy^2)) + 2 dmx dmy          the same with Cauchy-Schwarz on sum |x_i - m||y_i - m'|
 *   eA1 = 2 (|my| dmx + |mx| dmy + dmx dmy) + 2 u (2 |mx my| + c1)
 *   eB1 = 2 (|mx| dmx + |my| dmy) + dmx^2 + dmy^2 + 3 u B1
 *   eA2 = 2 esxy + 2 u (2 |sxy| + c2)            eB2 = esx + esy + 2 u B2
 *   eS  = (|A2| eA1 + |A1| eA2) / (B1 B2) + |S| (eB1 / B1 + eB2 / B2 + 3 u)
 *   forward    |err out| <= FN2I_BOUND_SLACK (eS + u |1 - S|) / 2
 * (the clamp moves nothing apart; FN2I_BOUND_SLACK = 1 + 2^-8 covers the products of two relative errors, each below 2^-17).
 * Gradient, per window p and with g = |g'| / n, dx = |x_q - mx_p|, dy = |y_q - my_p|, eE / E = eB1 / B1 + eB2 / B2 + 2 u:
 *   eDsxy = 2 E eA1 + |Dsxy| (eE / E + 2 u)                      eDs = eS / B2 + |Ds| (eB2 / B2 + u)
 *   eDmx  = 2 E (|A2| dmy + |my| eA2) + |2 my A2 E| (eE / E + 3 u) + 2 (|S| dmx + |mx| eS) / B1 + |2 mx S / B1| (eB1 / B1 + 3 u) + u |Dmx|
 *   tap_x = g (eDmx + 2 eDs dx + eDsxy dy + 2 |Ds| (dmx + u dx) + |Dsxy| (dmy + u dy)) + FN2I_BOUND_TAP u g (|Dmx| + 2 |Ds| dx + |Dsxy| dy)
 *   gradient   |err grad1[q]| <= FN2I_BOUND_SLACK sum_p w (tap_x + N1 u g |Dmx + 2 Ds (x_q - mx) + Dsxy (y_q - my)|)
 * (FN2I_BOUND_TAP = 8: the two products of gn, r, the products and the two additions of a tap; the last term the at most n - 1
 * additions of the gather over taps; grad2 by symmetry).  The bound presumes that pass is decided alike, that is |d| and |1 - d|
 * above the forward bound; at im2 == im1, the clamp's edge, both gradients are at most the bound in magnitude whichever side
 * rounding falls on.  These are worst cases: images of ordinary magnitude stay far below half of them.
 *
 * Kernels: a workgroup of 256 lanes owns FN2I_TILE_H x FN2I_TILE_W output pixels of one plane, a wave four rows of it, a lane four
 * vertically adjacent pixels of one column.  The forward stages both images' tile in LDS with md more rows above and below and
 * FN2I_HALO_X columns on either side, the backward with 2 md rows and 2 FN2I_HALO_X columns, through the reflected index in
 * reflect mode, as +0 outside the image in zero mode; with 16-byte loads where W is a multiple of 4 and the tensors are aligned
 * to 16 bytes (FN2I_HALO_X = 4 >= md keeps every patch row on a 16-byte boundary), one float at a time otherwise.  The backward
 * then forms the six maps Mx, My, A, B, mx, my of the windows within md of the tile in LDS (+0 for a window that is not valid)
 * and every pixel gathers from the k x k of them around it.  LDS:
 *   forward    FN2I_LDS_FWD(md) = 2 * 4 * (FN2I_TILE_H + 2 md) * (FN2I_TILE_W + 2 FN2I_HALO_X)                          (12672 B at md = 3)
 *   backward   FN2I_LDS_BWD(md) = 2 * 4 * (FN2I_TILE_H + 4 md) * (FN2I_TILE_W + 4 FN2I_HALO_X) + 6 * 4 * (FN2I_TILE_H + 2 md) * FN2I_MAP_PITCH
 *                                                                                                                    (55936 B at md = 3)
 * Every LDS access of the compute phases is a row segment of consecutive floats.  No scratch.
 *
 * Checks, all before a launch, in this order: N < 0 or C, H or W < 1 (FN2_EINVAL); a plane of 2^31 elements or more, 2^31 planes
 * or more, 2^48 elements or more or 2^31 workgroups or more (FN2_EUNSUPPORTED); the parameters: md not 1, 2 or 3, c1 or c2 not
 * finite or not > 0, border not 0 or 1, border reflect with H <= md or W <= md (FN2_EINVAL); N == 0 (FN2_OK, nothing launched);
 * a NULL im1, im2, out or grad_out, or grad1 and grad2 both NULL (FN2_EINVAL); a pointer not aligned to 4 bytes (FN2_EALIGN).
 */
#define FN2I_TILE_H 16
#define FN2I_TILE_W 64
#define FN2I_HALO_X 4
#define FN2I_MAP_PITCH 72
#define FN2I_MAX_DISTANCE 3
#define FN2I_BORDER_ZERO 0
#define FN2I_BORDER_REFLECT 1
#define FN2I_LDS_FWD(md) (2 * 4 * (FN2I_TILE_H + 2 * (md)) * (FN2I_TILE_W + 2 * FN2I_HALO_X))
#define FN2I_LDS_BWD(md) \
    (2 * 4 * (FN2I_TILE_H + 4 * (md)) * (FN2I_TILE_W + 4 * FN2I_HALO_X) + 6 * 4 * (FN2I_TILE_H + 2 * (md)) * FN2I_MAP_PITCH)
#define FN2I_BOUND_MEAN 1
#define FN2I_BOUND_MOMENT 4
#define FN2I_BOUND_TAP 8
#define FN2I_BOUND_SLACK (1.0 + 1.0 / 256)

int fn2i_ssim_forward(const void *im1, const void *im2, void *out, int N, int C, int H, int W, int md, float c1, float c2, int border,
                      void *stream);
int fn2i_ssim_backward(const void *im1, const void *im2, const void *grad_out, void *grad1, void *grad2, int N, int C, int H, int W,
                       int md, float c1, float c2, int border, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_SSIM_H */
