/*
 * flownet2_hip_ext.h -- C ABI of libflownet2_hip_ext.so: layers of the FlowNet family that are NOT among the reference's
 * three (Correlation, Resample2d, ChannelNorm) and therefore live outside the drop-in boundary of flownet2_hip.h.
 * Hand-written gfx950 (MI355X) HIP kernels, a library of its own: it links nothing of libflownet2_hip.so and adds nothing
 * to it.  Every name here starts with fn2x_.
 *
 * Conventions are those of flownet2_hip.h: NCHW device memory of the element type `dtype` names, `stream` is a hipStream_t
 * (work is enqueued on it, never synchronised), the caller has made the right device current, return value FN2_OK (0), a
 * negative FN2_E* code for a rejected call (nothing was launched) or a positive hipError_t from the launch.  Re-entrant, no
 * global mutable state.  Element-type values and return codes are the main header's; they are restated below under the same
 * names and values, so a translation unit may include both headers.
 */
#ifndef FLOWNET2_HIP_EXT_H
#define FLOWNET2_HIP_EXT_H

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FN2X_ABI_VERSION 1

#ifndef FLOWNET2_HIP_H
enum { FN2_F32 = 0, FN2_F16 = 1, FN2_F64 = 2, FN2_BF16 = 3 };
enum { FN2_OK = 0, FN2_EINVAL = -1, FN2_EDTYPE = -2, FN2_EALIGN = -3, FN2_EUNSUPPORTED = -4 };
#endif

int fn2x_abi_version(void); /* FN2X_ABI_VERSION */

/*
 * Correlation1d: the horizontal-search cost volume of stereo networks (DispNetC and its descendants; "Correlation1D" next to
 * the 2-D layer in the FlowNet 2.0 authors' code).  in1, in2: B x C x H x W, contiguous.
 *
 * Parameters: pad_size >= 0, max_displacement = md >= 0, stride1 = s1 >= 1, stride2 = s2 >= 1, single_direction = sd in
 * {-1, 0, +1}.  There is no kernel_size (it is 1).  With dr = md / s2 (integer division) the displacement index t runs over
 * -dr .. dr (sd = 0), -dr .. 0 (sd = -1) or 0 .. dr (sd = +1); output channel o = t - t_min, ascending;
 * nOut = 2 dr + 1 (sd = 0) or dr + 1.  oH = ceil(H / s1), oW = ceil((W + 2 pad - 2 md) / s1): padding is horizontal only.
 * oW < 1 is rejected (FN2_EINVAL), as the 2-D layer rejects an empty output.
 *
 *   out[b,o,y,x]      = (1/C) sum_c in1[b,c,y1,x1] * in2[b,c,y1,x1 + t s2],     y1 = y s1, x1 = x s1 + md - pad
 *   grad_in1[b,c,y,x] = (1/C) sum_t gO[b,o,y,x+pad-md]       * in2[b,c,y,x+t s2]
 *   grad_in2[b,c,y,x] = (1/C) sum_t gO[b,o,y,x-t s2+pad-md]  * in1[b,c,y,x-t s2]
 *
 * A term whose operand column (x1, x1 + t s2, x +- t s2) or output column lies outside is ABSENT, not a zero factor: an inf
 * next to the border does not make the outputs that pair it with the padding nan.  The backward supports stride1 == 1 only
 * (anything else: FN2_EUNSUPPORTED, as the 2-D layer).
 *
 * Arithmetic: that of FN2_CORR_DIRECT (flownet2_hip.h) for kernel_size 1, literally.  Forward: four partial sums over the
 * channels c mod 4 in ascending order, the C % 4 leftover channels appended to the first, 0 + ((s0 + s1) + (s2 + s3)), / C,
 * one rounding to T; half products are rounded to half, bf16 products are exact in fp32.  Backward: one sequential sum over
 * ascending t of (0 + gO) * v starting at +0, / C, one rounding.  Accumulators: fp32 for float, half and bf16; double tensors
 * accumulate in double in the backward and in float in the forward.  Multiply and add are two roundings.
 * Hence for pad_size == max_displacement, with D = 2 dr + 1: the forward for sd = 0 equals channels dr D .. (dr + 1) D - 1
 * (the centre row of the displacement window) of fn2_correlation_forward(kernel_size 1) BIT FOR BIT, and the backward
 * equals, for finite inputs and as numbers, the 2-D backward fed a gradOutput that is zero outside those channels.
 *
 * Per-element bounds (those of FN2_CORR_DIRECT with k = 1, n = nOut; S = the element's sum of |products| / C):
 *   forward  fp32: |out - exact| <= (floor(C/4) + C%4 + 4) 2^-23 S + 2^-23 |exact|
 *   backward fp32: |g - exact|   <= (nOut + 1) 2^-23 S + 2^-23 |exact|
 *   half / bf16  : the fp32 value within C 2^-23 S + 2^-23 |exact| (forward; half adds 2^-11 S + 2^-25 for its rounded
 *                  products) or nOut 2^-23 S + 2^-23 |exact| (backward) of the exact result, rounded once to the tensor's type.
 *
 * Selectors (`algo`):
 *   FN2X_CORR1D_GENERAL  one lane per output (forward) / input element (backward); any parameters; float, half, bf16, double.
 *   FN2X_CORR1D_TILED    LDS-tiled kernels (csrc/correlation_1d.hip).  Domain: stride1 == 1, stride2 == 1,
 *                        pad_size == max_displacement, 1 <= nOut <= 81 (md <= 40 two-sided, md <= 80 one-sided), float, half
 *                        or bf16, any B, C >= 1, H, W, element-aligned pointers, a batch item within 32-bit offsets
 *                        ((C + 4) H W and nOut H W below 2^31) and B <= 32767.  Outside it: FN2_EUNSUPPORTED, decided before
 *                        any launch.  Every element has the BITS of FN2X_CORR1D_GENERAL for the same call; where that
 *                        result is NaN the tiled one is NaN (payloads are not specified).
 *   FN2X_CORR1D_AUTO     backward: the tiled kernels wherever their domain holds (they split the channels over workgroups
 *                        and are measured 1.7 - 3.3 x faster at every size), else the general kernel.  Forward: the tiled
 *                        kernel where its domain holds AND nOut == 81 AND the call has at least 768 tiles of 32 x 4 pixels
 *                        over the whole batch (B ceil(W/32) ceil(H/4) >= 768; at B = 8: maps from 96 x 128 up); everything
 *                        else runs the general kernel, which is measured as fast or faster there: below that gate
 *                        (288 tiles: 1.0 x float, 0.7 - 0.9 x half / bf16) and for one-sided searches with nOut = 41 at any
 *                        measured size (0.65 - 0.9 x).  MI355X, B = 8, md 40: DESIGN.md 4.10, profiles/corr1d_micro.json.
 *                        Both paths give the same bits, so the gate is a matter of speed only.
 *   any other value: FN2_EINVAL.
 *
 * Checks, all before a launch, in this order: dtype (FN2_EDTYPE); shape and parameters, single_direction outside {-1, 0, 1},
 * an empty output (FN2_EINVAL); backward with stride1 != 1 (FN2_EUNSUPPORTED); B == 0 (FN2_OK, nothing launched); a NULL
 * pointer (FN2_EINVAL); a pointer not aligned to its element size (FN2_EALIGN); the selector.
 * Outputs are fully written; they need no pre-zeroing.
 */
enum { FN2X_CORR1D_AUTO = 0, FN2X_CORR1D_GENERAL = 1, FN2X_CORR1D_TILED = 2 };

int fn2x_correlation1d_output_shape(int H, int W, int pad_size, int max_displacement, int stride1, int stride2,
                                    int single_direction, int *nOut, int *oH, int *oW);
int fn2x_correlation1d_forward(const void *in1, const void *in2, void *out, int dtype, int B, int C, int H, int W,
                               int pad_size, int max_displacement, int stride1, int stride2, int single_direction,
                               int algo, void *stream);
int fn2x_correlation1d_backward(const void *in1, const void *in2, const void *grad_out, void *grad_in1, void *grad_in2,
                                int dtype, int B, int C, int H, int W, int pad_size, int max_displacement,
                                int stride1, int stride2, int single_direction, int algo, void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLOWNET2_HIP_EXT_H */
