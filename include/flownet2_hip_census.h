/*
 * flownet2_hip_census.h -- C ABI of libflownet2_hip_census.so: the ternary census distance, the photometric term of unsupervised
 * optical flow (UnFlow, ARFlow, UFlow, SMURF).  Each image is reduced to grey, every pixel is compared with the (2 md + 1)^2
 * patch around it through a soft sign, and the two images' soft census signatures are compared tap by tap through a robust
 * distance; the result is one plane per image pair.  Hand-written gfx950 (MI355X) HIP kernels, a library of its own: it links
 * none of libflownet2_hip.so, libflownet2_hip_ext.so, libflownet2_hip_lookup.so, libflownet2_hip_upsample.so,
 * libflownet2_hip_splat.so and adds nothing to them.  Every name here starts with fn2c_.
 *
 * Conventions are those of flownet2_hip.h: NCHW device memory, contiguous; `stream` is a hipStream_t (work is enqueued on it,
 * never synchronised), the caller has made the right device current, return value FN2_OK (0), a negative FN2_E* code for a
 * rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no global mutable state.
 * Return codes are the main header's, restated below under the same names and values (and left out if one of the other five
 * headers came first), so a translation unit may include all six headers, this one last.
 */
#ifndef FLOWNET2_HIP_CENSUS_H
#define FLOWNET2_HIP_CENSUS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2C_ABI_VERSION 1

#if !defined(FLOWNET2_HIP_H) && !defined(FLOWNET2_HIP_EXT_H) && !defined(FLOWNET2_HIP_LOOKUP_H) && !defined(FLOWNET2_HIP_UPSAMPLE_H) && \
    !defined(FLOWNET2_HIP_SPLAT_H)
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2c_abi_version(void); /* FN2C_ABI_VERSION */

/*
 * The operation.  im1, im2: N x C x H x W, float32, C = 1 or 3.  out: N x 1 x H x W, float32.  Parameters: max_distance md in
 * {1, 2, 3}, scale (finite; 255 for images in [0, 1]) and normalize.  P = 2 md + 1, K = P^2.  Every operation below is fp32,
 * rounded on its own, no contraction; csrc/census_arith.h holds it, host and device.
 *
 *   grey      C = 3: g = ((r 0.2989f + g 0.5870f) + b 0.1140f) scale        C = 1: g = v scale
 *   per tap   for pixel p and offset k = (dy, dx), |dy|, |dx| <= md, k != 0:
 *               x_i = g_i[p + k] - g_i[p]      r_i = rsq(0.81f + x_i x_i)      f_i = x_i r_i            (f(x) = x / sqrt(0.81 + x^2))
 *               d = f_1 - f_2                  h = (d d) rcp(0.1f + d d)                                (h(d) = d^2 / (0.1 + d^2))
 *   output    out[n, 0, p] = w sum_k h_k,  w = fl32(1 / K) if normalize (ARFlow's mean) else 1 (UFlow's sum).  The taps of one
 *             column dx are added in ascending dy starting from +0, then the columns' sums in ascending dx starting from +0.
 *   border    exactly +0 on the ring of width md around the image (ARFlow's valid mask): an interior pixel's patch never
 *             leaves the image.  An image with H < P or W < P is all ring: all +0.
 * rsq and rcp are the hardware's reciprocal square root and reciprocal (within 1 ulp).
 *
 * Backward, a gather: no atomics, no workspace, bit-reproducible.  gO' = grad_out inside the ring, +0 on it and outside the
 * image.  For pixel q and k != 0, with x_i = g_i[q] - g_i[q + k] (k and -k run over the same offsets; the grey of a pixel
 * outside the image counts as 0, and its term is 0 because both gO' are):
 *   s = gO'[q] + gO'[q + k]       t = s h'(d)       h'(d) = ((0.2f d) (q q)), q = rcp(0.1f + d d)       f'(x_i) = 0.81f ((r_i r_i) r_i)
 *   a1 += t f'(x_1)               a2 -= t f'(x_2)                     (per column dx from +0, then the columns, as the forward)
 *   grad_im_i[n, c, q] = (cw_c scale) (w a_i)       cw = (0.2989f, 0.5870f, 0.1140f) for C = 3, cw scale = scale for C = 1
 * One evaluation per pixel pair covers the pixel as centre and as neighbour: f is odd and f' is even.  Either gradient pointer
 * may be NULL (not wanted; both NULL is FN2_EINVAL); the one asked for alone has the bits it has in the pair.  Outputs are fully
 * written, no pre-zeroing.
 *
 * Domain: finite inputs with |g| < 2^60.  Anything else neither faults nor writes outside the outputs; its values are not pinned.
 *
 * Per-element bounds against the float64 evaluation on the fp32 grey intensities, u = 2^-24:
 *   out          |err| <= FN2C_FWD_BOUND w K,  FN2C_FWD_BOUND = 2^-19 = 32 u per tap.  Per tap: f_i carries 5 u (x^2, the sum,
 *                rsq 2 u, the product), d 12 u absolute, |h'| <= 2.06, h's own x^2, sum, rcp and product 6 u of h <= 1: below 31 u
 *                at the worst d; the column-wise summation adds at most 385 u sum h / 48.
 *   gradients    |err| <= FN2C_BWD_BOUND A(q, c),  FN2C_BWD_BOUND = 2^-15,
 *                A(q, c) = cw_c scale w sum_{k != 0} (|gO'[q]| + |gO'[q + k]|).  h'' <= 20 at d = 0, so h' carries 240 u from d and
 *                16 u of its own, f' <= 1.12 carries 13 u, the products and sums 40 u more: about 340 u = 2^-15.6 per term.
 *                Where A = 0 the gradient is exactly 0.
 * These are worst cases with every tap aligned; random images stay far below them.
 *
 * Kernels: a workgroup of 256 lanes owns FN2C_TILE_H x FN2C_TILE_W output pixels, a wave four rows of it, a lane four vertically
 * adjacent pixels of one column.  Both grey tiles with a halo of md are staged in LDS, converted to grey on the way (cells outside
 * the image are staged as 0, so the tap loop has no bounds test); the backward stages gO' the same way.  LDS:
 *   FN2C_LDS_BYTES(planes, md) = planes * 4 * (FN2C_TILE_H + 2 md) * (FN2C_TILE_W + 2 md + FN2C_PAD),  planes = 2 forward, 3 backward
 * (12496 B forward and 18744 B backward at md = 3).  Every LDS access of the tap loop is a row segment of 64 consecutive floats,
 * conflict-free at any pitch; FN2C_PAD = 1 makes the pitch odd so that a lane's column walk (rows y .. y + 3 + 2 md of one column)
 * does not return to a bank either.  No scratch.
 *
 * Checks, all before a launch, in this order: N < 0 or C, H or W < 1 (FN2_EINVAL); a plane of 2^31 elements or more, 2^31
 * planes or more, 2^48 elements or more in all, or 2^31 workgroups or more (FN2_EUNSUPPORTED); N == 0 (FN2_OK, nothing
 * launched); a NULL tensor pointer, in the backward both gradients NULL (FN2_EINVAL); a pointer not aligned to 4 bytes
 * (FN2_EALIGN); the parameters: C not 1 or 3, max_distance not 1, 2 or 3, scale not finite (FN2_EINVAL).
 */
#define FN2C_TILE_H 16
#define FN2C_TILE_W 64
#define FN2C_PAD 1
#define FN2C_MAX_DISTANCE 3
#define FN2C_LDS_BYTES(planes, md) ((planes) * 4 * (FN2C_TILE_H + 2 * (md)) * (FN2C_TILE_W + 2 * (md) + FN2C_PAD))
#define FN2C_FWD_BOUND_LOG2 -19
#define FN2C_BWD_BOUND_LOG2 -15

int fn2c_census_forward(const void *im1, const void *im2, void *out, int N, int C, int H, int W, int max_distance, float scale,
                        int normalize, void *stream);
int fn2c_census_backward(const void *im1, const void *im2, const void *grad_out, void *grad_im1, void *grad_im2, int N, int C, int H,
                         int W, int max_distance, float scale, int normalize, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_CENSUS_H */
