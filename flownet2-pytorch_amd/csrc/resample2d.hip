// resample2d.hip -- Resample2d (bilinear / nearest flow warp) forward and backward for gfx950.
//
// Replaces reference kernels kernel_resample2d_update_output (resample2d_kernel.cu:15-72),
// kernel_resample2d_backward_input1 (:75-125) and kernel_resample2d_backward_input2 (:127-198).
//
// HBM-bound gathers.  Unlike the reference (one thread per output ELEMENT: the flow is re-read
// and the weights re-derived once per channel), one lane owns PX consecutive output pixels and
// walks the image channels: flow is read once with a 16 B load, weights / corner offsets are
// formed once, every output plane gets a coalesced 16 B store.  Algorithmic bytes (fp32):
//   fwd  (2C + 2) * B*H*W * 4      bwd  (3C + 4) * B*H*W * 4  (+ the caller's zero-fill of grad_img)
// The backward pass is ONE kernel (the reference launches two, each re-reading flow, grad_out and
// the image): per pixel it scatters grad_out into the four corners of grad_img with hardware fp32
// atomics and forms both flow-gradient components from the same loaded corners.
// Arithmetic order follows the reference so the gather results are bit-identical to its source
// semantics: bilinear weights in double, each term rounded to float, float accumulation.
#include <algorithm>
#include <type_traits>

#include "fn2_common.h"
#include "resample2d_common.h"
#include "fn2_debug.h"
#include "corr_params.h"

namespace fn2 {

// ---------------------------------------------------------------- deterministic grad_input1: fixed-point accumulation
// The contract (include/flownet2_hip.h, fn2_resample2d_backward_det): per plane (b, c) of the scattered gradient, M = max |g|,
// E = frexp exponent of M, K = ceil(log2(16 k^2 H W)), s = 62 - E - K; every contribution v (the fp32 value the atomic path adds) becomes
// q = rne(v * 2^s) as an int64, the int64 sums are exact and order-free, and each cell gets g = g + (float)((double)Q * 2^-s).  Planes with
// an inf / NaN take a serial fp32 scatter instead (det_fallback).  Workspace: B*C plane maxima (|g| bits), then B*C planes of
// Hi x Wi int64 cells.
struct DetAcc {
    unsigned long long *acc;   // B*C planes of Hi*Wi int64 cells (two's complement in unsigned words: atomicAdd wraps the same way)
    const unsigned *pmax;      // B*C plane maxima, as the bits of |g|: >= 0x7f800000 = inf or NaN in the plane
    int K;
};

// E and s of a plane from its maximum's bits; false: the plane adds nothing here (all zero, or non-finite: the fallback's)
__device__ __forceinline__ bool det_scale(unsigned m, int K, int &s)
{
    if (m == 0u || m >= 0x7f800000u) return false;
    const int E = m >= 0x00800000u ? (int)(m >> 23) - 126 : (32 - __clz((int)m)) - 149;   // 2^(E-1) <= M < 2^E, subnormals included
    s = 62 - E - K;
    return true;
}
// q = round-to-nearest-even(v * 2^s): the scaling is exact in double (s may exceed fp32's exponent range), one rounding to int64
__device__ __forceinline__ unsigned long long det_q(float v, int s)
{
    return (unsigned long long)__double2ll_rn(ldexp((double)v, s));
}
__device__ __forceinline__ void det_add(unsigned long long *a, float v, int s) { atomicAdd(a, det_q(v, s)); }

// ---------------------------------------------------------------- forward
template <int PX>
__global__ __launch_bounds__(256) void resample_fwd_kernel(const float *__restrict__ img, ImgStrides is,
                                                           const float *__restrict__ flow, float *__restrict__ out,
                                                           int C, int Hi, int Wi, int H, int W, long ngroups,
                                                           int bilinear)
{
    const long HW = (long)H * W;
    const int gpr = W / PX; // groups per row (W % PX == 0 when PX > 1)
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < ngroups; g += (long)gridDim.x * blockDim.x) {
        const int x0 = (int)(g % gpr) * PX;
        const long row = g / gpr;
        const int y = (int)(row % H);
        const int b = (int)(row / H);
        const long fo = (long)b * 2 * HW + (long)y * W + x0;
        float dx[PX], dy[PX];
        if constexpr (PX == 4) {
            const f4 vx = *reinterpret_cast<const f4 *>(flow + fo);
            const f4 vy = *reinterpret_cast<const f4 *>(flow + fo + HW);
#pragma unroll
            for (int i = 0; i < 4; ++i) { dx[i] = vx[i]; dy[i] = vy[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < PX; ++i) { dx[i] = flow[fo + i]; dy[i] = flow[fo + HW + i]; }
        }
        long o00[PX], o01[PX], o10[PX], o11[PX];
        double w00[PX], w01[PX], w10[PX], w11[PX];
        // corners and weights written out: warp_fwd_corners / bilinear_weights here change the kernel's code
#pragma unroll
        for (int i = 0; i < PX; ++i) {
            const float xf = (float)(x0 + i) + dx[i], yf = (float)y + dy[i];
            if (bilinear) {
                const float fx = floorf(xf), fy = floorf(yf);
                const float alpha = xf - fx, beta = yf - fy; // (:45-46)
                // indices clamped with the OUTPUT dims (:49-52), then to the image (defensive)
                const int xL = clampi(clampi(f2i_sat(fx), 0, W - 1), 0, Wi - 1);
                const int xR = clampi(clampi(f2i_sat(fx + 1.0f), 0, W - 1), 0, Wi - 1);
                const int yT = clampi(clampi(f2i_sat(fy), 0, H - 1), 0, Hi - 1);
                const int yB = clampi(clampi(f2i_sat(fy + 1.0f), 0, H - 1), 0, Hi - 1);
                o00[i] = yT * is.h + xL * is.w;
                o01[i] = yT * is.h + xR * is.w;
                o10[i] = yB * is.h + xL * is.w;
                o11[i] = yB * is.h + xR * is.w;
                const double a = (double)alpha, be = (double)beta; // "1." literals -> double (:56-59)
                w00[i] = (1. - a) * (1. - be);
                w01[i] = a * (1. - be);
                w10[i] = (1. - a) * be;
                w11[i] = a * be;
            } else {
                // nearest: floor(xf + 0.5) in double (:66-67)
                const int xN = clampi(clampi(d2i_sat(floor((double)xf + 0.5)), 0, W - 1), 0, Wi - 1);
                const int yN = clampi(clampi(d2i_sat(floor((double)yf + 0.5)), 0, H - 1), 0, Hi - 1);
                o00[i] = yN * is.h + xN * is.w;
                o01[i] = o10[i] = o11[i] = o00[i];
                w00[i] = 1.;
                w01[i] = w10[i] = w11[i] = 0.;
            }
        }
        const float *ib = img + (long)b * is.b;
        float *ob = out + (long)b * C * HW + (long)y * W + x0;
        for (int c = 0; c < C; ++c) {
            const float *ic = ib + (long)c * is.c;
            float v[PX];
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const BilinearW w{w00[i], w01[i], w10[i], w11[i]};
                if (bilinear) v[i] = bilinear_sample(w, ic[o00[i]], ic[o01[i]], ic[o10[i]], ic[o11[i]]);
                else v[i] = ic[o00[i]];
            }
            if constexpr (PX == 4) {
                f4 r = {v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f4 *>(ob + (long)c * HW) = r;
            } else {
#pragma unroll
                for (int i = 0; i < PX; ++i) ob[(long)c * HW + i] = v[i];
            }
        }
    }
}

// ---------------------------------------------------------------- backward (fused input1 + input2)
// One lane per output pixel, lanes along x (coalesced flow / grad_out reads, coalesced grad_flow
// writes).  grad_img scatter: 4 fp32 hardware atomics per (pixel, channel); neighbouring lanes
// mostly hit neighbouring addresses, which the memory pipeline merges per cache line.
// DET: the deterministic mode -- the scatter adds fixed-point contributions to the workspace's int64 planes (DetAcc) instead of
// fp32 atomics to gimg; the gather is unchanged.
template <bool DET = false>
__global__ __launch_bounds__(256) void resample_bwd_kernel(const float *__restrict__ img, ImgStrides is,
                                                           const float *__restrict__ flow,
                                                           const float *__restrict__ gout,
                                                           float *__restrict__ gimg, float *__restrict__ gflow,
                                                           int C, int Hi, int Wi, int H, int W, long npix,
                                                           DetAcc det = DetAcc{})
{
    const long HW = (long)H * W, HWi = (long)Hi * Wi;
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < npix; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % W);
        const long row = g / W;
        const int y = (int)(row % H);
        const int b = (int)(row / H);
        const long p = (long)y * W + x;
        const float dx = flow[(long)b * 2 * HW + p], dy = flow[(long)b * 2 * HW + HW + p];
        int ixL, ixR, iyT, iyB;
        float alpha, beta, fa, fb;
        warp_bwd_pos(x, y, dx, dy, ixL, ixR, iyT, iyB, alpha, beta, fa, fb);

        // ---- grad_img: weights use truncation, alpha = xf - int(xf) (:105-106); corners clamped
        //      with the INPUT1 dims (:108-114); all float math (:118-121).
        const int sxL = clampi(ixL, 0, Wi - 1), sxR = clampi(ixR, 0, Wi - 1);
        const int syT = clampi(iyT, 0, Hi - 1), syB = clampi(iyB, 0, Hi - 1);
        const float s00 = (1 - alpha) * (1 - beta), s01 = alpha * (1 - beta);
        const float s10 = (1 - alpha) * beta, s11 = alpha * beta;

        // ---- grad_flow: corners clamped with the FLOW dims (:163-166) (then to the image, defensive)
        const int gxL = clampi(clampi(ixL, 0, W - 1), 0, Wi - 1), gxR = clampi(clampi(ixR, 0, W - 1), 0, Wi - 1);
        const int gyT = clampi(clampi(iyT, 0, H - 1), 0, Hi - 1), gyB = clampi(clampi(iyB, 0, H - 1), 0, Hi - 1);
        const float gam_y = 1 - fa, gam_x = 1 - fb;   // (:169, :182)
        float out_dx = 0.0f, out_dy = 0.0f;

        for (int ch = 0; ch < C; ++ch) {
            const float go = gout[((long)b * C + ch) * HW + p];
            if constexpr (DET) {
                int ds;
                if (det_scale(det.pmax[(long)b * C + ch], det.K, ds)) {
                    unsigned long long *A = det.acc + ((long)b * C + ch) * HWi;
                    det_add(A + (long)syT * Wi + sxL, s00 * go, ds);
                    det_add(A + (long)syT * Wi + sxR, s01 * go, ds);
                    det_add(A + (long)syB * Wi + sxL, s10 * go, ds);
                    det_add(A + (long)syB * Wi + sxR, s11 * go, ds);
                }
            } else {
                float *G = gimg + ((long)b * C + ch) * HWi;
                unsafeAtomicAdd(G + (long)syT * Wi + sxL, s00 * go);
                unsafeAtomicAdd(G + (long)syT * Wi + sxR, s01 * go);
                unsafeAtomicAdd(G + (long)syB * Wi + sxL, s10 * go);
                unsafeAtomicAdd(G + (long)syB * Wi + sxR, s11 * go);
            }

            const float *I = img + (long)b * is.b + (long)ch * is.c;
            const float iTL = I[gyT * is.h + gxL * is.w], iTR = I[gyT * is.h + gxR * is.w];
            const float iBL = I[gyB * is.h + gxL * is.w], iBR = I[gyB * is.h + gxR * is.w];
            flow_grad_terms(out_dx, out_dy, gam_x, gam_y, go, iTL, iTR, iBL, iBR);
        }
        gflow[(long)b * 2 * HW + p] = out_dx;
        gflow[(long)b * 2 * HW + HW + p] = out_dy;
    }
}

// ---------------------------------------------------------------- kernel_size > 1 (window sums)
// The reference adds the four corners at every offset (fy, fx) of a kernel_size x kernel_size window
// (resample2d_kernel.cu:54-61, :116-123) and, in the flow gradient, at the offsets 0 .. 2 * ((kernel_size-1)/2)
// (:171-178, :184-191) -- without any bounds test, i.e. it reads and accumulates outside its tensors near the lower
// and right borders.  Here the shifted indices are clamped to the image (the checker restates it the same way); wherever
// the reference stays inside its tensors the results are the reference's.  FlowNet2 only uses kernel_size 1
// (models.py:48,51), so these are plain one-lane-per-pixel kernels with the reference's operation order.
__global__ __launch_bounds__(256) void resample_fwd_ks_kernel(const float *__restrict__ img, ImgStrides is,
                                                              const float *__restrict__ flow, float *__restrict__ out,
                                                              int C, int Hi, int Wi, int H, int W, long npix, int ks, int bilinear)
{
    const long HW = (long)H * W;
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < npix; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % W);
        const long row = g / W;
        const int y = (int)(row % H);
        const int b = (int)(row / H);
        const long p = (long)y * W + x;
        const float dx = flow[(long)b * 2 * HW + p], dy = flow[(long)b * 2 * HW + HW + p];
        const float *ib = img + (long)b * is.b;
        float *ob = out + (long)b * C * HW + p;
        if (!bilinear) {   // nearest ignores kernel_size (:64-69)
            int xN, xR, yN, yB;
            float a = 0.0f, be = 0.0f;
            warp_fwd_corners(x, y, dx, dy, H, W, Hi, Wi, 0, xN, xR, yN, yB, a, be);
            for (int c = 0; c < C; ++c) ob[(long)c * HW] = ib[(long)c * is.c + yN * is.h + xN * is.w];
            continue;
        }
        const float xf = (float)x + dx, yf = (float)y + dy;
        const float fx0 = floorf(xf), fy0 = floorf(yf);
        // the flow's clamp only (the shifted corners are clamped to the image below); warp_pos here changes the kernel's code
        const int xL = clampi(f2i_sat(fx0), 0, W - 1), xR = clampi(f2i_sat(fx0 + 1.0f), 0, W - 1);
        const int yT = clampi(f2i_sat(fy0), 0, H - 1), yB = clampi(f2i_sat(fy0 + 1.0f), 0, H - 1);
        const BilinearW w = bilinear_weights(xf - fx0, yf - fy0);
        for (int c = 0; c < C; ++c) {
            const float *ic = ib + (long)c * is.c;
            float val = 0.0f;
            for (int fy = 0; fy < ks; ++fy)
                for (int fx = 0; fx < ks; ++fx) {
                    const long yt = clampi(yT + fy, 0, Hi - 1) * is.h, yb = clampi(yB + fy, 0, Hi - 1) * is.h;
                    const long xl = clampi(xL + fx, 0, Wi - 1) * is.w, xr = clampi(xR + fx, 0, Wi - 1) * is.w;
                    val = val + (float)(w.w00 * (double)ic[yt + xl]);   // one running sum over the window: not bilinear_sample's, which starts at 0
                    val = val + (float)(w.w01 * (double)ic[yt + xr]);
                    val = val + (float)(w.w10 * (double)ic[yb + xl]);
                    val = val + (float)(w.w11 * (double)ic[yb + xr]);
                }
            ob[(long)c * HW] = val;
        }
    }
}

template <bool DET = false>   // DET: as resample_bwd_kernel
__global__ __launch_bounds__(256) void resample_bwd_ks_kernel(const float *__restrict__ img, ImgStrides is,
                                                              const float *__restrict__ flow, const float *__restrict__ gout,
                                                              float *__restrict__ gimg, float *__restrict__ gflow,
                                                              int C, int Hi, int Wi, int H, int W, long npix, int ks,
                                                              DetAcc det = DetAcc{})
{
    const long HW = (long)H * W, HWi = (long)Hi * Wi;
    const int span = 2 * ((ks - 1) / 2);   // the flow gradient walks offsets 0 .. 2 * kernel_rad (:171, :184)
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < npix; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % W);
        const long row = g / W;
        const int y = (int)(row % H);
        const int b = (int)(row / H);
        const long p = (long)y * W + x;
        const float dx = flow[(long)b * 2 * HW + p], dy = flow[(long)b * 2 * HW + HW + p];
        int ixL, ixR, iyT, iyB;
        float alpha, beta, fa, fb;
        warp_bwd_pos(x, y, dx, dy, ixL, ixR, iyT, iyB, alpha, beta, fa, fb);
        // grad_img (:105-123): truncation weights, corners clamped with the image dims, float math
        const int sxL = clampi(ixL, 0, Wi - 1), sxR = clampi(ixR, 0, Wi - 1);
        const int syT = clampi(iyT, 0, Hi - 1), syB = clampi(iyB, 0, Hi - 1);
        const float s00 = (1 - alpha) * (1 - beta), s01 = alpha * (1 - beta), s10 = (1 - alpha) * beta, s11 = alpha * beta;
        for (int ch = 0; ch < C; ++ch) {
            const float go = gout[((long)b * C + ch) * HW + p];
            float *G = gimg + ((long)b * C + ch) * HWi;
            int ds = 0;
            if constexpr (DET) {
                if (!det_scale(det.pmax[(long)b * C + ch], det.K, ds)) continue;
            }
            for (int fy = 0; fy < ks; ++fy)
                for (int fx = 0; fx < ks; ++fx) {
                    const long yt = (long)clampi(syT + fy, 0, Hi - 1) * Wi, yb = (long)clampi(syB + fy, 0, Hi - 1) * Wi;
                    const int xl = clampi(sxL + fx, 0, Wi - 1), xr = clampi(sxR + fx, 0, Wi - 1);
                    if constexpr (DET) {
                        unsigned long long *A = det.acc + ((long)b * C + ch) * HWi;
                        det_add(A + yt + xl, s00 * go, ds);
                        det_add(A + yt + xr, s01 * go, ds);
                        det_add(A + yb + xl, s10 * go, ds);
                        det_add(A + yb + xr, s11 * go, ds);
                    } else {
                        unsafeAtomicAdd(G + yt + xl, s00 * go);
                        unsafeAtomicAdd(G + yt + xr, s01 * go);
                        unsafeAtomicAdd(G + yb + xl, s10 * go);
                        unsafeAtomicAdd(G + yb + xr, s11 * go);
                    }
                }
        }
        // grad_flow (:163-192): corners clamped with the flow dims, loops i (x offset), j (y offset), channel
        const int gxL = clampi(ixL, 0, W - 1), gxR = clampi(ixR, 0, W - 1), gyT = clampi(iyT, 0, H - 1), gyB = clampi(iyB, 0, H - 1);
        const float gam_y = 1 - fa, gam_x = 1 - fb;   // (:169, :182)
        float out_dx = 0.0f, out_dy = 0.0f;
        for (int i = 0; i <= span; ++i)
            for (int j = 0; j <= span; ++j)
                for (int ch = 0; ch < C; ++ch) {
                    const float go = gout[((long)b * C + ch) * HW + p];
                    const float *I = img + (long)b * is.b + (long)ch * is.c;
                    const long yb = clampi(gyB + j, 0, Hi - 1) * is.h, yt = clampi(gyT + j, 0, Hi - 1) * is.h;
                    const long xl = clampi(gxL + i, 0, Wi - 1) * is.w, xr = clampi(gxR + i, 0, Wi - 1) * is.w;
                    const float iTL = I[yt + xl], iTR = I[yt + xr], iBL = I[yb + xl], iBR = I[yb + xr];
                    flow_grad_terms(out_dx, out_dy, gam_x, gam_y, go, iTL, iTR, iBL, iBR);
                }
        gflow[(long)b * 2 * HW + p] = out_dx;
        gflow[(long)b * 2 * HW + HW + p] = out_dy;
    }
}

// ---------------------------------------------------------------- tiled kernels (LDS windows)
// With an arbitrary flow every lane of a wave gathers from / scatters to a different cache line; the per-CU
// vector-memory path then moves a 64-128 B line per 4 useful bytes, and device-scope fp32 atomics to scattered
// addresses leave the XCD (the per-XCD L2s are not coherent) at a few tens of G atomics/s.  The tiled kernels
// give a workgroup a TH x TW tile of output / source pixels and an LDS window covering the tile +- R pixels:
//   forward : the image window is loaded with coalesced 16 B loads, one channel at a time, and the four
//             bilinear corners are gathered from LDS; samples whose corners leave the window read global memory
//   backward: per channel, an image window (for the flow gradient's corner differences) and an accumulation
//             window: the four-corner scatter goes to LDS (compare-and-swap adds), only out-of-window targets use global
//             atomics, and the window is flushed as contiguous rows (exact zeros skipped) -- the windows of
//             neighbouring tiles overlap, so the flush accumulates too.
// Arithmetic and operation order are those of the reference kernels (see resample_fwd_kernel /
// resample_bwd_kernel above, which remain as the fallback for small images and strided pixel layouts).
// fp32 accumulation into LDS.  The native ds_add_f32 runs at ~0.33 lane-atomics/clk/CU on gfx950 (measured,
// scripts/ubench/lds_atomics.hip: integer LDS atomics reach 7-11), a compare-and-swap loop on the same word
// reaches ~2.5 -- 7x faster for the scattered, rarely colliding adds of the warp gradient.
__device__ __forceinline__ void lds_add_f32(float *addr, float v)
{
    unsigned *a = reinterpret_cast<unsigned *>(addr);
    unsigned old = *a, assumed;
    do {
        assumed = old;
        old = atomicCAS(a, assumed, __float_as_uint(__uint_as_float(assumed) + v));
    } while (old != assumed);
}

// fp64 cell += fp32 value: ds_add_f64 without return (the product was formed in fp32 as the reference forms it; the
// conversion is exact)
__device__ __forceinline__ void lds_add_f64(double *addr, float v)
{
    __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double *)addr, (double)v);
}
__device__ __forceinline__ void lds_add_f64(float *, float) {}   // never called (ACC 0 instantiations)

// FUSE (models.py:133-138): `img` is the second image of a B x 2C x H x W pair tensor `pair`, and the
// kernel writes cat((pair, warped, flow / div_flow, ||pair[:, :C] - warped||_2), 1) = B x (3C+3) x H x W in one pass:
// the warped channel, the copy of both images (the second one comes from the LDS window), the squared difference
// accumulated in channel order as channelnorm_kernel.cu:41-52 does, then the flow and the norm planes.
template <int TH, int TW, int R, int FUSE = 0>   // 0: Resample2d; 1: row N2's concat; 2: the norm plane only (models.py:157-161)
__global__ __launch_bounds__(1024, 8) void resample_fwd_tiled(const float *__restrict__ img, ImgStrides is,
                                                            const float *__restrict__ flow, float *__restrict__ out,
                                                            int C, int Hi, int Wi, int H, int W, int tiles_x, int tiles_y,
                                                            int bilinear, const float *__restrict__ pair = nullptr,
                                                            float div_flow = 1.0f)
{
    // 1024 threads, <= 64 VGPRs: two workgroups (32 waves) per CU.  Per-pixel state is 4 registers: the four corners are
    // base + {0, dx, dy*stride, both} (clamping can only merge neighbours) and the double-precision weights are rebuilt per
    // channel from alpha/beta with the reference's expressions.  The window is double-buffered: channel c+1 is loaded to
    // registers before channel c is gathered and written to the other buffer afterwards -- one barrier per channel.
    constexpr int NT = 1024, WH = TH + 2 * R, WW = TW + 2 * R, PPT = TH * TW / NT;
    __shared__ __attribute__((aligned(16))) float win[2][WH * WW];
    enum { LIVE = 1, IN_WIN = 2, DX = 4, DY = 8 };

    const int tid = threadIdx.x;
    int t = (int)xcd_remap(blockIdx.x, gridDim.x);   // an XCD's workgroups take consecutive tiles: neighbours share its L2
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int X0 = tx * TW, Y0 = ty * TH, wx0 = X0 - R, wy0 = Y0 - R;
    const long HW = (long)H * W;

    float alpha[PPT], beta[PPT];
    float ssq[FUSE ? PPT : 1];
    int base[PPT], flags[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        if (FUSE) ssq[k] = 0.0f;
        alpha[k] = beta[k] = 0.0f;
        base[k] = flags[k] = 0;
        if (!((x < W) && (y < H))) continue;
        const long p = (long)y * W + x;
        const float dx = flow[(long)b * 2 * HW + p], dy = flow[(long)b * 2 * HW + HW + p];
        int xL, xR, yT, yB;
        warp_fwd_corners(x, y, dx, dy, H, W, Hi, Wi, bilinear, xL, xR, yT, yB, alpha[k], beta[k]);
        const int lxL = xL - wx0, lxR = xR - wx0, lyT = yT - wy0, lyB = yB - wy0;
        const bool in = (lxL >= 0) && (lxR < WW) && (lyT >= 0) && (lyB < WH);
        base[k] = in ? lyT * WW + lxL : yT * (int)is.h + xL * (int)is.w;
        flags[k] = LIVE | (in ? IN_WIN : 0) | (xR != xL ? DX : 0) | (yB != yT ? DY : 0);
    }

    // window rows are contiguous in the image (pixel stride 1 and Wi % 4 == 0 are launcher preconditions): 16 B per
    // lane, a 4-px group is entirely inside or outside the image
    constexpr int NW = (WH * (WW / 4) + NT - 1) / NT;
    f4 wreg[NW];
    auto win_load = [&](const float *I) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            int i = tid + NT * j;
            asm volatile("" : "+v"(i));    // keep the address arithmetic inside the channel loop (register budget)
            const int ly = i / (WW / 4), lx = (i - ly * (WW / 4)) * 4;
            const int gy = wy0 + ly, gx = wx0 + lx;
            f4 v = (f4){0.0f, 0.0f, 0.0f, 0.0f};
            if (i < WH * (WW / 4) && gy >= 0 && gy < Hi && gx >= 0 && gx < Wi)
                v = *reinterpret_cast<const f4 *>(I + (long)gy * is.h + gx);
            wreg[j] = v;
        }
    };
    auto win_write = [&](float *dst) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = tid + NT * j;
            if (i < WH * (WW / 4)) *reinterpret_cast<f4 *>(dst + 4 * i) = wreg[j];
        }
    };
    if (C > 0) { win_load(img + (long)b * is.b); win_write(win[0]); }
    __syncthreads();

    for (int c = 0; c < C; ++c) {
        const float *I = img + (long)b * is.b + (long)c * is.c;
        const float *wc = win[c & 1];
        if (c + 1 < C) win_load(I + is.c);
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            int fl = flags[k], o = base[k], idx = tid + NT * k;
            if (!(fl & LIVE)) continue;
            asm volatile("" : "+v"(fl), "+v"(o), "+v"(idx));   // as above
            const int x = X0 + idx % TW, y = Y0 + idx / TW;
            float i00, i01, i10, i11;
            if (fl & IN_WIN) {
                const int ox = (fl & DX) ? 1 : 0, oy = (fl & DY) ? WW : 0;
                i00 = wc[o]; i01 = wc[o + ox]; i10 = wc[o + oy]; i11 = wc[o + oy + ox];
            } else {
                const int ox = (fl & DX) ? (int)is.w : 0, oy = (fl & DY) ? (int)is.h : 0;
                i00 = I[o]; i01 = I[o + ox]; i10 = I[o + oy]; i11 = I[o + oy + ox];
            }
            const float val = bilinear ? bilinear_sample(alpha[k], beta[k], i00, i01, i10, i11) : i00;
            if (!FUSE) store_out(out + ((long)b * C + c) * HW + (y * W + x), val);
            else {
                const int pix = y * W + x;
                const float v0 = pair[((long)b * 2 * C + c) * HW + pix];
                if (FUSE == 1) {
                    float *ob = out + (long)b * (3 * C + 3) * HW + pix;
                    const float v1 = wc[(y - wy0) * WW + (x - wx0)];        // the pixel itself is always inside the window
                    store_out(ob + (long)c * HW, v0);
                    store_out(ob + (long)(C + c) * HW, v1);
                    store_out(ob + (long)(2 * C + c) * HW, val);
                }
                const float d = v0 - val;                               // models.py:134
                ssq[k] = ssq[k] + d * d;                                // channelnorm_kernel.cu:47-50
            }
        }
        if (c + 1 < C) win_write(win[(c + 1) & 1]);
        __syncthreads();
    }
    if (FUSE) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int idx = tid + NT * k;
            const int x = X0 + idx % TW, y = Y0 + idx / TW;
            if (!(flags[k] & LIVE)) continue;
            const int pix = y * W + x;
            if (FUSE == 2) {                                            // only ||first image - warped||: B x 1 x H x W
                store_out(out + (long)b * HW + pix, sqrtf(ssq[k]));
                continue;
            }
            float *ob = out + (long)b * (3 * C + 3) * HW + pix;
            // models.py:138 `flow / self.div_flow` on a GPU tensor: PyTorch multiplies by the fp32 reciprocal of a scalar divisor
            const float inv_div = 1.0f / div_flow;
            store_out(ob + (long)(3 * C) * HW, flow[(long)b * 2 * HW + pix] * inv_div);
            store_out(ob + (long)(3 * C + 1) * HW, flow[(long)b * 2 * HW + HW + pix] * inv_div);
            store_out(ob + (long)(3 * C + 2) * HW, sqrtf(ssq[k]));                      // channelnorm_kernel.cu:52
        }
    }
}

// Forward, 4 ADJACENT pixels per thread: the flow arrives as two 16-byte loads and every output plane leaves as one 16-byte store per
// thread (resample_fwd_tiled: 4-byte accesses strided by the workgroup size -- four times the vector-memory instructions for the
// same bytes, and the CU's vector-memory path retires instructions, not bytes: ~33 cycles each inside a kernel).
// TH x 64 tile, TH * 16 threads; window double-buffered per channel as in resample_fwd_tiled.
template <int TH, int R>
__global__ __launch_bounds__(TH * 16, (2 * TH * 16 + 255) / 256) void resample_fwd_tiled4(const float *__restrict__ img, ImgStrides is,
                                                                                        const float *__restrict__ flow, float *__restrict__ out,
                                                                                        int C, int Hi, int Wi, int H, int W, int tiles_x, int tiles_y,
                                                                                        int bilinear)
{
    constexpr int TW = 64, NT = TH * 16, WH = TH + 2 * R, WW = TW + 2 * R, NW = (WH * (WW / 4) + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) float win[2][WH * WW];
    enum { IN_WIN = 2, DX = 4, DY = 8 };
    const int tid = threadIdx.x;
    int t = (int)xcd_remap(blockIdx.x, gridDim.x);   // an XCD's workgroups take consecutive tiles: neighbours share its L2
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int X0 = tx * TW, Y0 = ty * TH, wx0 = X0 - R, wy0 = Y0 - R;
    const long HW = (long)H * W;
    const int x0 = X0 + 4 * (tid & 15), y = Y0 + (tid >> 4);
    const bool live = x0 < W && y < H;                        // W % 4 == 0: a group is entirely inside or outside
    const long p0 = live ? (long)y * W + x0 : 0;
    const f4 vdx = *reinterpret_cast<const f4 *>(flow + (long)b * 2 * HW + p0);
    const f4 vdy = *reinterpret_cast<const f4 *>(flow + (long)b * 2 * HW + HW + p0);
    f4 wreg[NW];
    auto win_load = [&](const float *I) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            int i = tid + NT * j;
            asm volatile("" : "+v"(i));
            const int ly = i / (WW / 4), lx = (i - ly * (WW / 4)) * 4;
            const int gy = wy0 + ly, gx = wx0 + lx;
            f4 v = (f4){0.0f, 0.0f, 0.0f, 0.0f};
            if (i < WH * (WW / 4) && gy >= 0 && gy < Hi && gx >= 0 && gx < Wi)
                v = *reinterpret_cast<const f4 *>(I + (long)gy * is.h + gx);
            wreg[j] = v;
        }
    };
    auto win_write = [&](float *dst) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = tid + NT * j;
            if (i < WH * (WW / 4)) *reinterpret_cast<f4 *>(dst + 4 * i) = wreg[j];
        }
    };
    if (C > 0) win_load(img + (long)b * is.b);
    float alpha[4], beta[4];
    int base[4], flags[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int xL, xR, yT, yB;
        alpha[k] = beta[k] = 0.0f;
        warp_fwd_corners(x0 + k, y, vdx[k], vdy[k], H, W, Hi, Wi, bilinear, xL, xR, yT, yB, alpha[k], beta[k]);
        const int lxL = xL - wx0, lxR = xR - wx0, lyT = yT - wy0, lyB = yB - wy0;
        const bool in = (lxL >= 0) && (lxR < WW) && (lyT >= 0) && (lyB < WH);
        base[k] = in ? lyT * WW + lxL : yT * (int)is.h + xL * (int)is.w;
        flags[k] = (in ? IN_WIN : 0) | (xR != xL ? DX : 0) | (yB != yT ? DY : 0);
    }
    if (C > 0) win_write(win[0]);
    __syncthreads();
    for (int c = 0; c < C; ++c) {
        const float *I = img + (long)b * is.b + (long)c * is.c;
        const float *wc = win[c & 1];
        if (c + 1 < C) win_load(I + is.c);
        f4 res;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int fl = flags[k], o = base[k];
            asm volatile("" : "+v"(fl), "+v"(o));
            float i00, i01, i10, i11;
            if (fl & IN_WIN) {
                const int ox = (fl & DX) ? 1 : 0, oy = (fl & DY) ? WW : 0;
                i00 = wc[o]; i01 = wc[o + ox]; i10 = wc[o + oy]; i11 = wc[o + oy + ox];
            } else {
                const int ox = (fl & DX) ? (int)is.w : 0, oy = (fl & DY) ? (int)is.h : 0;
                i00 = I[o]; i01 = I[o + ox]; i10 = I[o + oy]; i11 = I[o + oy + ox];
            }
            const float val = bilinear ? bilinear_sample(alpha[k], beta[k], i00, i01, i10, i11) : i00;
            res[k] = val;
        }
        if (live) store_out(reinterpret_cast<f4 *>(out + ((long)b * C + c) * HW + p0), res);
        if (c + 1 < C) win_write(win[(c + 1) & 1]);
        __syncthreads();
    }
}

// Forward with ALL image channels of the window resident in LDS (C == NC, typically 3): a workgroup owns a TH x TW tile,
// loads the NC windows at once (one barrier in the whole kernel instead of one per channel), forms the corner offsets and the
// double-precision weights once per pixel and gathers the NC channels back to back.
// One tile of the all-channel forward: rows [Y0, Y0 + TH) x columns [X0, X0 + TW) of item b; `win` holds NC windows of
// (TH + 2R) x (TW + 2R) floats.  The caller provides the barrier before `win` is reused.
template <int TH, int TW, int R, int NC, int NT>
__device__ __forceinline__ void fwd_tile_all(float *__restrict__ win, const float *__restrict__ img, const ImgStrides is,
                                             const float *__restrict__ flow, float *__restrict__ out, int Hi, int Wi, int H, int W,
                                             int b, int X0, int Y0, int ylim, int bilinear, unsigned long long *ts = nullptr)
{
    // `ts` (profiling, debug library): four wall-clock stamps (100 MHz) -- entry, windows written to LDS, barrier, stores issued
    constexpr int WH = TH + 2 * R, WW = TW + 2 * R, PPT = TH * TW / NT, NW = (WH * (WW / 4) + NT - 1) / NT;
    static_assert(TH * TW % NT == 0, "whole pixels per thread");
    const int tid = threadIdx.x;
    if (ts) ts[0] = wall_clock64();
    const int wx0 = X0 - R, wy0 = Y0 - R;
    const long HW = (long)H * W;
    // the flow of the thread's pixels and every window group: all requested before anything is used
    float fdx[PPT], fdy[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        const long p = (x < W && y < ylim) ? (long)y * W + x : 0;
        fdx[k] = flow[(long)b * 2 * HW + p]; fdy[k] = flow[(long)b * 2 * HW + HW + p];
    }
    f4 wreg[NC][NW];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = tid + NT * j;
            const int ly = i / (WW / 4), lx = (i - ly * (WW / 4)) * 4;
            const int gy = wy0 + ly, gx = wx0 + lx;
            f4 v = (f4){0.0f, 0.0f, 0.0f, 0.0f};
            if (i < WH * (WW / 4) && gy >= 0 && gy < Hi && gx >= 0 && gx < Wi)
                v = *reinterpret_cast<const f4 *>(img + (long)b * is.b + (long)c * is.c + (long)gy * is.h + gx);
            wreg[c][j] = v;
        }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = tid + NT * j;
            if (i < WH * (WW / 4)) *reinterpret_cast<f4 *>(win + c * (WH * WW) + 4 * i) = wreg[c][j];
        }
    if (ts) ts[1] = wall_clock64();
    __syncthreads();
    if (ts) ts[2] = wall_clock64();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        if (!((x < W) && (y < ylim))) continue;
        int xL, xR, yT, yB;
        float alpha = 0.0f, beta = 0.0f;
        warp_fwd_corners(x, y, fdx[k], fdy[k], H, W, Hi, Wi, bilinear, xL, xR, yT, yB, alpha, beta);
        const int lxL = xL - wx0, lxR = xR - wx0, lyT = yT - wy0, lyB = yB - wy0;
        const bool in = (lxL >= 0) && (lxR < WW) && (lyT >= 0) && (lyB < WH);
        const BilinearW w = bilinear_weights(alpha, beta);
        const int o = in ? lyT * WW + lxL : yT * (int)is.h + xL * (int)is.w;
        const int ox = (xR != xL) ? (in ? 1 : (int)is.w) : 0, oy = (yB != yT) ? (in ? WW : (int)is.h) : 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float i00, i01, i10, i11;
            if (in) {
                const float *wc = win + c * (WH * WW);
                i00 = wc[o]; i01 = wc[o + ox]; i10 = wc[o + oy]; i11 = wc[o + oy + ox];
            } else {
                const float *I = img + (long)b * is.b + (long)c * is.c;
                i00 = I[o]; i01 = I[o + ox]; i10 = I[o + oy]; i11 = I[o + oy + ox];
            }
            store_out(out + ((long)b * NC + c) * HW + (y * W + x), bilinear ? bilinear_sample(w, i00, i01, i10, i11) : i00);
        }
    }
    if (ts) ts[3] = wall_clock64();
}

template <int TH, int TW, int R, int NC, int WPE = 4, int NTH = 1024>
__global__ __launch_bounds__(NTH, WPE) void resample_fwd_tiled_all(const float *__restrict__ img, ImgStrides is,
                                                                const float *__restrict__ flow, float *__restrict__ out,
                                                                int Hi, int Wi, int H, int W, int tiles_x, int tiles_y, int bilinear,
                                                                unsigned long long *dbg = nullptr)
{
    __shared__ __attribute__((aligned(16))) float win[NC * (TH + 2 * R) * (TW + 2 * R)];
    int t = (int)xcd_remap(blockIdx.x, gridDim.x);   // an XCD's workgroups take consecutive tiles: neighbours share its L2
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    unsigned long long ts[4] = {0, 0, 0, 0};
    fwd_tile_all<TH, TW, R, NC, NTH>(win, img, is, flow, out, Hi, Wi, H, W, t / tiles_y, tx * TW, ty * TH, H, bilinear, dbg ? ts : nullptr);
    if (dbg && threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned long long *d = dbg + (long)blockIdx.x * 8;
        for (int i = 0; i < 4; ++i) d[i] = ts[i];
        d[4] = wall_clock64();
    }
}

// The backward windows FOLLOW the flow.  A tile's accumulation / image window is tile +- R px around where the tile's pixels LAND,
// not around the tile: real flow fields are locally smooth but not small (FlowNet2 warps by the estimated motion, tens of pixels on
// Sintel), and with a window centred on the tile a translation of (25, -18) px sends every corner to the global-atomic path -- 760 us
// instead of 38 for the same field without the translation (8 x 3 x 384 x 512).  The offset is a robust centre of the flow at four
// pixels of the tile (its quadrant centres): per component the mean of the two middle values if they
// agree, so that one or two outliers among the four change nothing -- the plain mean moved 4 % of the tiles of the SURVEY's white-noise flow (1 % of its
// values are x20) far away from their pixels: 51 -> 77 us.  It is rounded -- to a multiple of 4 px in x, so that the 16-byte groups of
// the image window stay aligned -- and zero below 8 px, which leaves small flows exactly where they were.  Only the placement of the
// window depends on it; which pixels take the LDS path never changes a result beyond the order of the fp32 sums of grad_input1.
struct TileFlowSample { float v; };   // lane l holds component (l >> 2) & 1 of sample pixel l & 3
__device__ __forceinline__ void tile_flow_sample(const float *__restrict__ flow_b, long HW, int X0, int Y0, int TW, int TH, int H, int W,
                                                 TileFlowSample &S)
{
    // ONE vector load per wave (eight scalar loads per wave through the scalar cache cost the kernel 4 us)
    const int l = threadIdx.x & 7, q = l & 3;
    const int sx = min(X0 + TW / 4 + (q & 1) * (TW / 2), W - 1), sy = min(Y0 + TH / 4 + (q >> 1) * (TH / 2), H - 1);
    S.v = flow_b[((l >> 2) ? HW : 0) + (long)sy * W + sx];
}
// the two middle values of four: their mean if they agree within 8 px, else "no estimate" (two of the four were outliers)
__device__ __forceinline__ float middle_of_four(const float v[4])
{
    const float a = fminf(v[0], v[1]), b = fmaxf(v[0], v[1]), c = fminf(v[2], v[3]), d = fmaxf(v[2], v[3]);
    const float m1 = fmaxf(a, c), m2 = fminf(b, d);
    return fabsf(m1 - m2) < 8.0f ? 0.5f * (m1 + m2) : 0.0f;
}
__device__ __forceinline__ void tile_window_offset(const TileFlowSample &S, int &offx, int &offy, int xq = 4)
{
    float sx[4], sy[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sx[q] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(S.v), q));
        sy[q] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(S.v), 4 + q));
    }
    const float mx = middle_of_four(sx), my = middle_of_four(sy);
    offx = (fabsf(mx) >= 8.0f && fabsf(mx) < 1.0e6f) ? xq * (int)rintf(mx / (float)xq) : 0;   // xq = 4 or 16: exact divisions
    offy = (fabsf(my) >= 8.0f && fabsf(my) < 1.0e6f) ? (int)rintf(my) : 0;
}

template <int TH, int TW, int R, int NT, int WPE, int ACC = 0>
__global__ __launch_bounds__(NT, WPE) void resample_bwd_tiled(const float *__restrict__ img, ImgStrides is,
                                                            const float *__restrict__ flow,
                                                            const float *__restrict__ gout,
                                                            float *__restrict__ gimg, float *__restrict__ gflow,
                                                            int C, int Hi, int Wi, int H, int W, int tiles_x, int tiles_y,
                                                            int abl,   // abl: profiling switches (0 in production)
                                                            DetAcc det = DetAcc{})   // ACC 2 only
{
    // Two workgroups per CU (<= 64 VGPRs, 2 x 49 KB LDS): one workgroup's window loads overlap the other's LDS scatter.
    // Per-pixel state is therefore kept small: the four corners are base + {0, dx, dy*stride, both} with dx, dy in {0,1}
    // (clamping can only merge neighbours), and the bilinear weights are recomputed per channel from alpha/beta with the
    // reference's expressions.
    constexpr int WH = TH + 2 * R, WW = TW + 2 * R, WWP = WW + 1, PPT = TH * TW / NT;
    __shared__ __attribute__((aligned(16))) float iwin[WH * WW];   // image window
    // accumulation window (+1: rows on different banks).  ACC 0: fp32 cells, added to with a compare-and-swap loop (lds_add_f32);
    // ACC 1: fp64 cells, added to with ds_add_f64 -- no return value, no retry loop, no round trip per add (the returning LDS
    // atomic is what bounds the CAS loop, scripts/ubench/lds_cas_pipelined.hip); the sum is rounded to fp32 once, at the flush.
    // ACC 2: the deterministic mode -- int64 fixed-point cells (same bytes as fp64), ds_add_u64 in LDS, 64-bit integer atomics into the
    // workspace's accumulator planes for far pixels and the flush; grad_img itself is written by the conversion pass.
    typedef std::conditional_t<ACC == 2, unsigned long long, std::conditional_t<ACC == 1, double, float>> acc_t;
    __shared__ acc_t awin[WH * WWP];
    enum { LIVE = 1, S_IN = 2, G_IN = 4, S_DX = 8, S_DY = 16, G_DX = 32, G_DY = 64 };

    const int tid = threadIdx.x;
    int t = (int)xcd_remap(blockIdx.x, gridDim.x);   // an XCD's workgroups take consecutive tiles: neighbours share its L2
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int b = t / tiles_y;
    const int X0 = tx * TW, Y0 = ty * TH;
    const long HW = (long)H * W, HWi = (long)Hi * Wi;
    TileFlowSample tfs;
    tile_flow_sample(flow + (long)b * 2 * HW, HW, X0, Y0, TW, TH, H, W, tfs);
    int wx0, wy0;   // set below, once the thread's own loads have been requested

    // per-pixel state (flow is read once)
    float alpha[PPT], beta[PPT], gam_x[PPT], gam_y[PPT], out_dx[PPT], out_dy[PPT];
    int sbase[PPT], gbase[PPT], flags[PPT];
    // image-window staging: a thread owns NW 4-px groups; loaded to registers (so the loads of channel c+1 are in flight
    // while channel c's accumulation window is flushed), then written to LDS
    constexpr int NW = (WH * (WW / 4) + NT - 1) / NT;
    f4 wreg[NW];
    auto win_load = [&](const float *I) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            int i = tid + NT * j;
            asm volatile("" : "+v"(i));    // keep the address arithmetic inside the channel loop (register budget)
            const int ly = i / (WW / 4), lx = (i - ly * (WW / 4)) * 4;
            const int gy = wy0 + ly, gx = wx0 + lx;
            f4 v = (f4){0.0f, 0.0f, 0.0f, 0.0f};
            // Wi % 4 == 0 (launcher): a 4-px group is entirely inside or outside the image
            if (i < WH * (WW / 4) && gy >= 0 && gy < Hi && gx >= 0 && gx < Wi)
                v = *reinterpret_cast<const f4 *>(I + (long)gy * is.h + gx);
            wreg[j] = v;
        }
    };
    auto win_write = [&]() {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = tid + NT * j;
            if (i < WH * (WW / 4)) *reinterpret_cast<f4 *>(iwin + 4 * i) = wreg[j];
        }
    };
    // all flow values of the thread are requested before the first one is used (one memory round trip instead of PPT); the
    // window's place follows from the tile's flow sample, requested before them, and the first image window goes out right behind
    float fdx[PPT], fdy[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        const bool in = (x < W) && (y < H);
        const long p = in ? (long)y * W + x : 0;
        fdx[k] = flow[(long)b * 2 * HW + p]; fdy[k] = flow[(long)b * 2 * HW + HW + p];
    }
    wx0 = X0 - R; wy0 = Y0 - R;
    if (C > 0) win_load(img + (long)b * is.b);
    __builtin_amdgcn_sched_barrier(0);
    {   // requested where the tile is, and once more if the flow sample says its pixels land elsewhere (never for flows below 8 px)
        int offx, offy;
        tile_window_offset(tfs, offx, offy);
        if (offx | offy) {
            wx0 += offx; wy0 += offy;
            if (C > 0) win_load(img + (long)b * is.b);
        }
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        out_dx[k] = out_dy[k] = 0.0f;
        alpha[k] = beta[k] = gam_x[k] = gam_y[k] = 0.0f;
        sbase[k] = gbase[k] = 0;
        flags[k] = 0;
        if (!((x < W) && (y < H))) continue;
        int fl = LIVE;
        const float dx = fdx[k], dy = fdy[k];
        int ixL, ixR, iyT, iyB;
        float fa, fb;
        warp_bwd_pos(x, y, dx, dy, ixL, ixR, iyT, iyB, alpha[k], beta[k], fa, fb);
        gam_y[k] = 1 - fa; gam_x[k] = 1 - fb;   // (:169, :182)
        {   // scatter corners: clamped with the INPUT1 dims (:108-114)
            const int xL = clampi(ixL, 0, Wi - 1), xR = clampi(ixR, 0, Wi - 1);
            const int yT = clampi(iyT, 0, Hi - 1), yB = clampi(iyB, 0, Hi - 1);
            const int lxL = xL - wx0, lxR = xR - wx0, lyT = yT - wy0, lyB = yB - wy0;
            const bool in = (lxL >= 0) && (lxR < WW) && (lyT >= 0) && (lyB < WH);
            sbase[k] = in ? lyT * WWP + lxL : yT * Wi + xL;
            fl |= (in ? S_IN : 0) | (xR != xL ? S_DX : 0) | (yB != yT ? S_DY : 0);
        }
        {   // gather corners: clamped with the FLOW dims (:163-166), then to the image
            const int xL = clampi(clampi(ixL, 0, W - 1), 0, Wi - 1), xR = clampi(clampi(ixR, 0, W - 1), 0, Wi - 1);
            const int yT = clampi(clampi(iyT, 0, H - 1), 0, Hi - 1), yB = clampi(clampi(iyB, 0, H - 1), 0, Hi - 1);
            const int lxL = xL - wx0, lxR = xR - wx0, lyT = yT - wy0, lyB = yB - wy0;
            const bool in = (lxL >= 0) && (lxR < WW) && (lyT >= 0) && (lyB < WH);
            gbase[k] = in ? lyT * WW + lxL : yT * (int)is.h + xL * (int)is.w;
            fl |= (in ? G_IN : 0) | (xR != xL ? G_DX : 0) | (yB != yT ? G_DY : 0);
        }
        flags[k] = fl;
        __builtin_amdgcn_sched_barrier(0);
    }

    for (int i = tid; i < WH * WWP; i += NT) awin[i] = (acc_t)0;
    win_write();
    __syncthreads();

    for (int c = 0; c < C; ++c) {
        const float *I = img + (long)b * is.b + (long)c * is.c;
        float *G = gimg + ((long)b * C + c) * HWi;
        int ds = 0;                 // ACC 2: the plane's scale exponent; dq false = nothing to add for this plane
        bool dq = true;
        unsigned long long *A = nullptr;
        if constexpr (ACC == 2) {
            dq = det_scale(det.pmax[(long)b * C + c], det.K, ds);
            A = det.acc + ((long)b * C + c) * HWi;
        }
        float gov[PPT];   // the channel's grad_out values of the thread: requested together (one round trip, not PPT)
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            int idx = tid + NT * k;
            asm volatile("" : "+v"(idx));
            const int x = X0 + idx % TW, y = Y0 + idx / TW;
            gov[k] = (flags[k] & LIVE) ? gout[((long)b * C + c) * HW + (y * W + x)] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            int fl = flags[k], sb = sbase[k], gb = gbase[k];
            if (!(fl & LIVE)) continue;
            // opaque to the optimiser: otherwise every corner address of every pixel is hoisted out of the channel
            // loop and the kernel no longer fits the 64 VGPRs two workgroups per CU need
            asm volatile("" : "+v"(fl), "+v"(sb), "+v"(gb));
            const float go = gov[k];
            const float s00 = (1 - alpha[k]) * (1 - beta[k]), s01 = alpha[k] * (1 - beta[k]);
            const float s10 = (1 - alpha[k]) * beta[k], s11 = alpha[k] * beta[k];
            if ((abl & 2) || !dq) {
            } else if (fl & S_IN) {
                const int ox = (fl & S_DX) ? 1 : 0, oy = (fl & S_DY) ? WWP : 0;
                if constexpr (ACC == 2) {
                    det_add(awin + sb, s00 * go, ds);
                    det_add(awin + sb + ox, s01 * go, ds);
                    det_add(awin + sb + oy, s10 * go, ds);
                    det_add(awin + sb + oy + ox, s11 * go, ds);
                } else if constexpr (ACC == 1) {
                    lds_add_f64(awin + sb, s00 * go);
                    lds_add_f64(awin + sb + ox, s01 * go);
                    lds_add_f64(awin + sb + oy, s10 * go);
                    lds_add_f64(awin + sb + oy + ox, s11 * go);
                } else {
                    lds_add_f32(awin + sb, s00 * go);
                    lds_add_f32(awin + sb + ox, s01 * go);
                    lds_add_f32(awin + sb + oy, s10 * go);
                    lds_add_f32(awin + sb + oy + ox, s11 * go);
                }
            } else if constexpr (ACC == 2) {
                const int ox = (fl & S_DX) ? 1 : 0, oy = (fl & S_DY) ? Wi : 0;
                det_add(A + sb, s00 * go, ds);
                det_add(A + sb + ox, s01 * go, ds);
                det_add(A + sb + oy, s10 * go, ds);
                det_add(A + sb + oy + ox, s11 * go, ds);
            } else {
                const int ox = (fl & S_DX) ? 1 : 0, oy = (fl & S_DY) ? Wi : 0;
                unsafeAtomicAdd(G + sb, s00 * go);
                unsafeAtomicAdd(G + sb + ox, s01 * go);
                unsafeAtomicAdd(G + sb + oy, s10 * go);
                unsafeAtomicAdd(G + sb + oy + ox, s11 * go);
            }
            float iTL, iTR, iBL, iBR;
            if (abl & 4) { iTL = iTR = iBL = iBR = go; }
            else if (fl & G_IN) {
                const int ox = (fl & G_DX) ? 1 : 0, oy = (fl & G_DY) ? WW : 0;
                iTL = iwin[gb]; iTR = iwin[gb + ox]; iBL = iwin[gb + oy]; iBR = iwin[gb + oy + ox];
            } else {
                const int ox = (fl & G_DX) ? (int)is.w : 0, oy = (fl & G_DY) ? (int)is.h : 0;
                iTL = I[gb]; iTR = I[gb + ox]; iBL = I[gb + oy]; iBR = I[gb + oy + ox];
            }
            // written out: flow_grad_terms here changes the code of the wider profiling instantiations
            out_dy[k] = out_dy[k] + (gam_y[k] * go) * iBL;       // (:172-177)
            out_dy[k] = out_dy[k] - (gam_y[k] * go) * iTL;
            out_dy[k] = out_dy[k] + ((1 - gam_y[k]) * go) * iBR;
            out_dy[k] = out_dy[k] - ((1 - gam_y[k]) * go) * iTR;
            out_dx[k] = out_dx[k] + (gam_x[k] * go) * iTR;       // (:185-190)
            out_dx[k] = out_dx[k] - (gam_x[k] * go) * iTL;
            out_dx[k] = out_dx[k] + ((1 - gam_x[k]) * go) * iBR;
            out_dx[k] = out_dx[k] - ((1 - gam_x[k]) * go) * iBL;
            __builtin_amdgcn_sched_barrier(0);   // one pixel at a time: keeps the live set small
        }
        __syncthreads();
        if (c + 1 < C) win_load(I + is.c);
        // flush the accumulation window as contiguous rows (exact zeros skipped) and clear it for the next channel
        {
            int ly = tid / WW, lx = tid - ly * WW;     // element tid, then steps of NT without divisions
#pragma unroll 2
            for (int i = tid; i < WH * WW; i += NT) {
                const int gx = wx0 + lx, gy = wy0 + ly;
                const acc_t v = awin[ly * WWP + lx];
                if (v != (acc_t)0) {
                    awin[ly * WWP + lx] = (acc_t)0;
                    if (!(abl & 1) && gx >= 0 && gx < Wi && gy >= 0 && gy < Hi) {
                        if constexpr (ACC == 2) atomicAdd(A + gy * Wi + gx, v);
                        else unsafeAtomicAdd(G + gy * Wi + gx, (float)v);
                    }
                }
                ly += NT / WW; lx += NT % WW;
                if (lx >= WW) { lx -= WW; ++ly; }
            }
        }
        if (c + 1 < C) win_write();
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        if (!(flags[k] & LIVE)) continue;
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        const long p = (long)y * W + x;
        store_out(gflow + (long)b * 2 * HW + p, out_dx[k]);
        store_out(gflow + (long)b * 2 * HW + HW + p, out_dy[k]);
    }
}

// ---------------------------------------------------------------- backward, three channels in one scatter
// resample_bwd_tiled above walks the channels one at a time: per channel it rebuilds the weights and corner addresses of
// every pixel, scatters, flushes, and reloads the image window -- seven barriers for C = 3.  FlowNet2 only warps 3-channel
// images (models.py:133-174), so this variant keeps ALL THREE accumulation windows in LDS (fp32 cells, 3 x 24.8 KB = 74.5 KB:
// still two workgroups per CU): a pixel's weights and addresses are formed once and its adds issued back to back --
// channels 0 and 1 of a cell share one 64-bit word updated by ONE compare-and-swap, channel 2 has a word of its own: 8 LDS
// atomics per pixel instead of 12 --; one flush pass; then the three image windows take the same LDS bytes and grad_flow is
// gathered for all channels.  Four barriers.  Arithmetic and operation order per output as resample_bwd_tiled with fp32 cells
// (the kernel of round 3); grad_flow is bit-identical to it.
// Measured (scripts/resample_micro.py, 8 x 3 x 384 x 512, us; white-noise / smooth flow): loads, barriers and zeroing alone
// 17 (resample_bwd_tiled: 26), + scatter 14 / 10, + flush 19 / 12: the flush is the largest part (why: the atomic-request bound in
// the kernel's own comment below).  (Half of the workgroups running the gather first, so that their flushes pass
// under the others' scatters, gained 3 us on the smooth flow and nothing on the white-noise one, and the kernel's time moved by
// +-3 us with the mere layout of that second path's code: one order, straight-line text.)
__device__ __forceinline__ void lds_add_f32x2(unsigned long long *a, float v0, float v1)
{
    // (starting from an assumed 0 instead of this read -- a third of the adds find an untouched cell -- measured 1 us slower:
    // a failed compare-and-swap costs more than the read it replaces, profiles/r05_e_caszero.log)
    unsigned long long old = *a, assumed;
    do {
        assumed = old;
        const float lo = __uint_as_float((unsigned)assumed) + v0, hi = __uint_as_float((unsigned)(assumed >> 32)) + v1;
        old = atomicCAS(a, assumed, ((unsigned long long)__float_as_uint(hi) << 32) | __float_as_uint(lo));
    } while (old != assumed);
}

// The 12 adds of one pixel into the three accumulation windows.  `pile`: a corner was clamped to the image border in a wave where
// at least 8 lanes were -- clamping sends whole runs of pixels to ONE cell (a translation of 25 px puts 25 lanes of a wave on the last
// column; the stray outlier of a noisy flow does not count: a wave that takes this path pays for it with all its lanes).  A
// compare-and-swap loop retries once per colliding lane and a round trip each -- 790 us for the translated field of tile_window_offset's note --, so these
// pixels use the LDS's own fp32 add: 0.33 lane-atomics/clk/CU, 7x slower than the loop without collisions, but collisions are
// resolved inside the LDS unit.  It may touch one half of a 64-bit pair another lane updates by compare-and-swap: both are single
// LDS operations, and the swap fails and retries if the word changed under it.
__device__ __forceinline__ void c3_add_pixel(unsigned long long *a01, float *a2, int sb, int ox, int oy, float s00, float s01,
                                             float s10, float s11, float g0, float g1, float g2, bool pile)
{
    if (!pile) {
        lds_add_f32x2(a01 + sb, s00 * g0, s00 * g1);
        lds_add_f32x2(a01 + sb + ox, s01 * g0, s01 * g1);
        lds_add_f32x2(a01 + sb + oy, s10 * g0, s10 * g1);
        lds_add_f32x2(a01 + sb + oy + ox, s11 * g0, s11 * g1);
        lds_add_f32(a2 + sb, s00 * g2);
        lds_add_f32(a2 + sb + ox, s01 * g2);
        lds_add_f32(a2 + sb + oy, s10 * g2);
        lds_add_f32(a2 + sb + oy + ox, s11 * g2);
    } else {
        // corners that clamping merged into one cell are added once (their weights summed first: the reference issues them as
        // separate atomics in no particular order)
        typedef __attribute__((address_space(3))) float lds_float;
        lds_float *p01 = (lds_float *)a01, *p2 = (lds_float *)a2;
        float a = s00, b = s01, c = s10, d = s11;
        if (!ox) { a += b; c += d; }
        if (!oy) { a += c; b += d; }
        auto add = [&](int cell, float w) {
            __builtin_amdgcn_ds_faddf(p01 + 2 * cell, w * g0, 0, 0, false);
            __builtin_amdgcn_ds_faddf(p01 + 2 * cell + 1, w * g1, 0, 0, false);
            __builtin_amdgcn_ds_faddf(p2 + cell, w * g2, 0, 0, false);
        };
        add(sb, a);
        if (ox) add(sb + ox, b);
        if (oy) add(sb + oy, c);
        if (ox && oy) add(sb + oy + ox, d);
    }
}

// ---------------------------------------------------------------- backward, three channels: the kernel
// The scheme described above (all three accumulation windows in LDS, one scatter, one flush, then the image windows and the gather),
// its inputs in one argument block, and two options (round 5):
//   FUSED (row N2, models.py:133-138 differentiated): the gradient of the warped image is formed on the fly from the concat
//     gradient -- g_warped = g_cat[6:9] - g_norm * diff / (norm + 1e-9) (channelnorm_kernel.cu:93), diff = first image - warped
//     image read back from the forward's concat buffer --, the first image's gradient g_cat[0:3] + g_diff is written on the way, and
//     the flow gradient gets the flow / div_flow term added;
//   SCATTER = false when the image pair needs no gradient (it is the network's input): gather only, no LDS atomics, no global
//     atomics, 73.7 KB of LDS.
// The window is aligned to 64 bytes in x (tile_window_offset rounds to 16 px here): a flushed row is 6 atomic requests, never 7.
// What bounds the scattering form (scripts/ubench/atomic_rate.hip, flush_probe.hip): global fp32 atomics on gfx950 are
// performed outside the XCD whatever their scope -- workgroup and agent scope have ONE encoding, and the rate does not depend
// on which XCDs share an image -- at ~20.5 G REQUESTS/s chip-wide, a request being the lanes of one instruction that fall into one
// aligned 64-byte segment (16 consecutive floats cost what a single float costs).  8 x 3 x 384 x 512 with the white-noise flow:
// 0.59 M flush requests + 0.20 M from the 18 k far pixels = 39 us of atomic-unit time, which cannot start before the first
// windows are complete (timeline, scripts/resample_timeline.py: loads 3 us, then the scatter -- 33 k LDS compare-and-swap pairs per CU
// at 2.5 per clock: 8-13 us): 50-53 us.  (Delaying the second workgroup of every CU by 2-10 us so that one scatters while the other
// flushes changes nothing: 53.1-54.7 us, profiles/r05_d_resample_stagger.log.)  Measured and dropped in round 5 (scripts/attic/resample_bwd_fill_farlist.hip.txt,
// profiles/r05_b_resample_fill_farlist.log): far pixels collected in an LDS list and issued with the two corners of a row in
// adjacent lanes (half the far requests, but issued in the flush phase instead of trickling out while the atomic unit idles:
// 59.6 us against 52.7) and the zero fill of grad_input1 folded into the kernel behind claim / completion counters (four
// dependent memory round trips per workgroup cost more than the 5.7 us fill they replace: 69.0 us against 58.1 with the fill).
// Arithmetic and operation order per output as resample_bwd_tiled with fp32 cells; grad_flow is bit-identical to it.
struct C3xArgs {
    const float *img; ImgStrides is;          // the image that was warped (FUSED: pair + 3 HW, batch stride 6 HW)
    const float *flow;
    const float *gout;                        // !FUSED: B x 3 x H x W gradient of the warped image
    const float *gcat, *pair, *outcat;        // FUSED: B x 12 x H x W concat gradient, B x 6 x H x W images, B x 12 x H x W forward output
    float *gpair0;                            // FUSED: B x 6 x H x W gradient of the pair (channels 0..2 written here), or null
    float *gimg; long gimg_bs;                // scatter target, 3 planes of Hi x Wi per item, gimg_bs floats between items
    float *gflow;
    int B, Hi, Wi, H, W, tiles_x, tiles_y, abl;
    int bilinear;                             // FUSED == 2: how the forward sampled (its value is recomputed)
    float inv_div_flow;
    unsigned long long *dbg;                  // profiling (abl & 8): the debug library's stamp buffer (fn2_debug_set_buffer), else null
};

template <int FUSED>
__device__ __forceinline__ void c3x_load_go(const C3xArgs &p, int b, long pix, long HW, float go[3], bool write_gpair0)
{
    if constexpr (FUSED == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) go[c] = p.gout[((long)b * 3 + c) * HW + pix];
    } else if constexpr (FUSED == 2) {   // the first image's pixel: the gradient is formed at the gather, from the recomputed warp
#pragma unroll
        for (int c = 0; c < 3; ++c) go[c] = p.pair[((long)b * 6 + c) * HW + pix];
    } else {
        const float gn = p.gcat[((long)b * 12 + 11) * HW + pix], nrm = p.outcat[((long)b * 12 + 11) * HW + pix];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float diff = p.pair[((long)b * 6 + c) * HW + pix] - p.outcat[((long)b * 12 + 6 + c) * HW + pix];   // (models.py:134)
            const float gd = chnorm_grad(gn, diff, nrm);
            go[c] = p.gcat[((long)b * 12 + 6 + c) * HW + pix] - gd;
            if (write_gpair0 && p.gpair0) store_out(p.gpair0 + ((long)b * 6 + c) * HW + pix, p.gcat[((long)b * 12 + c) * HW + pix] + gd);
        }
    }
}

// FUSED: 0 = Resample2d's backward; 1 = row N2's concat (above); 2 = the norm-only form (models.py:157-161, :170-174:
// ||first image - warped||_2 with no concat): gcat / outcat are the B x 1 x H x W gradient of the norm and the norm, the warped image
// was never stored and is recomputed at the gather from the same corners with the forward's arithmetic; gather only (SCATTER false).
template <int TH, int TW, int R, int NT, int FUSED, bool SCATTER>
__global__ __launch_bounds__(NT, 8) void resample_bwd_c3x(const C3xArgs p)
{
    static_assert(FUSED != 2 || !SCATTER, "the norm-only form is gather-only");
    constexpr int WH = TH + 2 * R, WW = TW + 2 * R, WWP = WW + 1, PPT = TH * TW / NT, CELLS = WH * WWP, C = 3;
    constexpr int NW = (WH * (WW / 4) + NT - 1) / NT;
    constexpr int WIN_BYTES = SCATTER ? CELLS * 12 : 3 * WH * WW * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[WIN_BYTES];
    float *const aw = reinterpret_cast<float *>(smem);
    unsigned long long *const a01 = reinterpret_cast<unsigned long long *>(smem);
    float *const a2 = reinterpret_cast<float *>(smem + CELLS * 8);
    float *const iwin = reinterpret_cast<float *>(smem);
    static_assert(3 * WH * WW * 4 <= WIN_BYTES, "image windows must fit the accumulation windows' bytes");
    enum { LIVE = 1, G_IN = 4, G_DX = 32, G_DY = 64 };

    const int tid = threadIdx.x;
    int t = (int)xcd_remap(blockIdx.x, gridDim.x);
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y;
    const int b = t / p.tiles_y;
    const int X0 = tx * TW, Y0 = ty * TH;
    const int H = p.H, W = p.W, Hi = p.Hi, Wi = p.Wi;
    const long HW = (long)H * W, HWi = (long)Hi * Wi;
    const ImgStrides is = p.is;
    const float *const img = p.img;
    float *const gimg_b = p.gimg + (long)b * p.gimg_bs;
    TileFlowSample tfs;
    tile_flow_sample(p.flow + (long)b * 2 * HW, HW, X0, Y0, TW, TH, H, W, tfs);
    // profiling (abl & 8, debug library only): wall-clock stamps (100 MHz) of the workgroup's phases, dumped into the debug buffer
    unsigned long long ts[6] = {0, 0, 0, 0, 0, 0};
    auto stamp = [&](int i) __attribute__((always_inline)) { if ((p.abl & 8) && p.dbg) ts[i] = wall_clock64(); };
    stamp(0);

    float fdx[PPT], fdy[PPT], go[PPT][C];
    float gnv[FUSED == 2 ? PPT : 1], nrv[FUSED == 2 ? PPT : 1], alv[FUSED == 2 ? PPT : 1], btv[FUSED == 2 ? PPT : 1];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        const bool live = (x < W) && (y < H);
        const long pix = live ? (long)y * W + x : 0;
        fdx[k] = p.flow[(long)b * 2 * HW + pix]; fdy[k] = p.flow[(long)b * 2 * HW + HW + pix];
        c3x_load_go<FUSED>(p, b, pix, HW, go[k], live);
        if (FUSED == 2) { gnv[k] = p.gcat[(long)b * HW + pix]; nrv[k] = p.outcat[(long)b * HW + pix]; }
    }
    if (SCATTER)
        for (int i = tid; i < CELLS * 3; i += NT) aw[i] = 0.0f;
    __builtin_amdgcn_sched_barrier(0);   // all of that goes out before the wave waits for its flow sample
    int offx, offy;
    // 16-px steps where a window is flushed (a flushed row is then exactly six 64-byte segments); the gather-only instantiations have no
    // flush to align and keep the finer 4-px steps (2 instead of 8 px of the margin lost at worst: ADVICE r5)
    tile_window_offset(tfs, offx, offy, SCATTER ? 16 : 4);
    const int wx0 = X0 - R + offx, wy0 = Y0 - R + offy;
    if (SCATTER) __syncthreads();
    stamp(1);

    float gam_x[PPT], gam_y[PPT];
    int gbase[PPT], flags[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        gam_x[k] = gam_y[k] = 0.0f;
        gbase[k] = flags[k] = 0;
        if (!((x < W) && (y < H))) continue;
        int fl = LIVE;
        // written out: warp_bwd_pos forms the scatter's alpha / beta ahead of the `continue` below, which reorders this kernel's code
        const float xf = (float)x + fdx[k], yf = (float)y + fdy[k];
        const float fx = floorf(xf), fy = floorf(yf);
        const int ixL = f2i_sat(fx), ixR = f2i_sat(fx + 1.0f), iyT = f2i_sat(fy), iyB = f2i_sat(fy + 1.0f);
        gam_y[k] = 1 - (xf - fx);   // c == 1 branch (:169)
        gam_x[k] = 1 - (yf - fy);   // c == 0 branch (:182)
        if (FUSED == 2) { alv[k] = xf - fx; btv[k] = yf - fy; }   // the forward's alpha, beta (resample2d_kernel.cu:45-46)
        {   // gather corners: clamped with the FLOW dims (:163-166), then to the image
            const int xL = clampi(clampi(ixL, 0, W - 1), 0, Wi - 1), xR = clampi(clampi(ixR, 0, W - 1), 0, Wi - 1);
            const int yT = clampi(clampi(iyT, 0, H - 1), 0, Hi - 1), yB = clampi(clampi(iyB, 0, H - 1), 0, Hi - 1);
            const int lxL = xL - wx0, lxR = xR - wx0, lyT = yT - wy0, lyB = yB - wy0;
            const bool in = (lxL >= 0) && (lxR < WW) && (lyT >= 0) && (lyB < WH);
            gbase[k] = in ? lyT * WW + lxL : yT * (int)is.h + xL * (int)is.w;
            fl |= (in ? G_IN : 0) | (xR != xL ? G_DX : 0) | (yB != yT ? G_DY : 0);
        }
        flags[k] = fl;
        if (!SCATTER || (p.abl & 2)) continue;
        // scatter: weights by truncation (:105-106), corners clamped with the INPUT1 dims (:108-114)
        const float alpha = xf - (float)f2i_sat(xf), beta = yf - (float)f2i_sat(yf);
        const float s00 = (1 - alpha) * (1 - beta), s01 = alpha * (1 - beta), s10 = (1 - alpha) * beta, s11 = alpha * beta;
        const int xL = clampi(ixL, 0, Wi - 1), xR = clampi(ixR, 0, Wi - 1), yT = clampi(iyT, 0, Hi - 1), yB = clampi(iyB, 0, Hi - 1);
        const int lxL = xL - wx0, lxR = xR - wx0, lyT = yT - wy0, lyB = yB - wy0;
        if ((lxL >= 0) && (lxR < WW) && (lyT >= 0) && (lyB < WH)) {
            const int sb = lyT * WWP + lxL, ox = (xR != xL) ? 1 : 0, oy = (yB != yT) ? WWP : 0;
            const bool moved = (xL != ixL) || (xR != ixR) || (yT != iyT) || (yB != iyB);   // a corner was clamped to the border
            c3_add_pixel(a01, a2, sb, ox, oy, s00, s01, s10, s11, go[k][0], go[k][1], go[k][2],
                         moved && __popcll(__ballot(moved)) >= 8);
        } else {
            // far pixel: 12 atomics now, while the atomic unit has nothing else to do (the flushes come later)
            const int sb = yT * Wi + xL, ox = (xR != xL) ? 1 : 0, oy = (yB != yT) ? Wi : 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float *G = gimg_b + (long)c * HWi + sb;
                unsafeAtomicAdd(G, s00 * go[k][c]);
                unsafeAtomicAdd(G + ox, s01 * go[k][c]);
                unsafeAtomicAdd(G + oy, s10 * go[k][c]);
                unsafeAtomicAdd(G + oy + ox, s11 * go[k][c]);
            }
        }
    }
    if (SCATTER) __syncthreads();
    stamp(2);

    // the three image windows are requested now: their latency passes under the flush
    f4 wreg[C][NW];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = tid + NT * j;
            const int ly = i / (WW / 4), lx = (i - ly * (WW / 4)) * 4;
            const int gy = wy0 + ly, gx = wx0 + lx;
            f4 v = (f4){0.0f, 0.0f, 0.0f, 0.0f};
            if (i < WH * (WW / 4) && gy >= 0 && gy < Hi && gx >= 0 && gx < Wi)
                v = *reinterpret_cast<const f4 *>(img + (long)b * is.b + (long)c * is.c + (long)gy * is.h + gx);
            wreg[c][j] = v;
        }
    if constexpr (SCATTER) {
        if (!(p.abl & 1)) {
            int ly = tid / WW, lx = tid - ly * WW;
#pragma unroll 2
            for (int i = tid; i < WH * WW; i += NT) {
                const int gx = wx0 + lx, gy = wy0 + ly;
                const int cell = ly * WWP + lx;
                float v0, v1, v2;
                {
                    const unsigned long long u = a01[cell];
                    v0 = __uint_as_float((unsigned)u); v1 = __uint_as_float((unsigned)(u >> 32)); v2 = a2[cell];
                }
                if (gx >= 0 && gx < Wi && gy >= 0 && gy < Hi) {
                    float *G = gimg_b + gy * Wi + gx;
                    if (v0 != 0.0f) unsafeAtomicAdd(G, v0);
                    if (v1 != 0.0f) unsafeAtomicAdd(G + HWi, v1);
                    if (v2 != 0.0f) unsafeAtomicAdd(G + 2 * HWi, v2);
                }
                ly += NT / WW; lx += NT % WW;
                if (lx >= WW) { lx -= WW; ++ly; }
            }
        }
        stamp(3);      // flush atomics issued (not retired: they return nothing)
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = tid + NT * j;
            if (i < WH * (WW / 4)) *reinterpret_cast<f4 *>(iwin + c * (WH * WW) + 4 * i) = wreg[c][j];
        }
    __syncthreads();
    stamp(4);

#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int fl = flags[k], gb = gbase[k];
        if (!(fl & LIVE)) continue;
        float out_dx = 0.0f, out_dy = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float g = go[k][c];
            float iTL, iTR, iBL, iBR;
            if (p.abl & 4) { iTL = iTR = iBL = iBR = g; }
            else if (fl & G_IN) {
                const float *wc = iwin + c * (WH * WW);
                const int ox = (fl & G_DX) ? 1 : 0, oy = (fl & G_DY) ? WW : 0;
                iTL = wc[gb]; iTR = wc[gb + ox]; iBL = wc[gb + oy]; iBR = wc[gb + oy + ox];
            } else {
                const float *I = img + (long)b * is.b + (long)c * is.c;
                const int ox = (fl & G_DX) ? (int)is.w : 0, oy = (fl & G_DY) ? (int)is.h : 0;
                iTL = I[gb]; iTR = I[gb + ox]; iBL = I[gb + oy]; iBR = I[gb + oy + ox];
            }
            if constexpr (FUSED == 2) {
                // the forward's sample (resample2d_kernel.cu:56-59 / :66-69) from the same four corners, then ChannelNorm's gradient of
                // the difference (channelnorm_kernel.cu:93) with the sign of d(diff)/d(warped)
                float val;   // warp_value<true>, written out: the helper (or bilinear_sample alone) reorders this kernel's code
                if (p.bilinear) {
                    const double a = (double)alv[k], be = (double)btv[k];
                    val = 0.0f;
                    val = val + (float)(((1. - a) * (1. - be)) * (double)iTL);
                    val = val + (float)((a * (1. - be)) * (double)iTR);
                    val = val + (float)(((1. - a) * be) * (double)iBL);
                    val = val + (float)((a * be) * (double)iBR);
                } else {
                    val = alv[k] >= 0.5f ? (btv[k] >= 0.5f ? iBR : iTR) : (btv[k] >= 0.5f ? iBL : iTL);
                }
                g = 0.0f - chnorm_grad(gnv[k], g - val, nrv[k]);
            }
            flow_grad_terms(out_dx, out_dy, gam_x[k], gam_y[k], g, iTL, iTR, iBL, iBR);
        }
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        const long pix = (long)y * W + x;
        if (FUSED == 1) {   // + the gradient through flow / div_flow = flow * (1 / div_flow) (models.py:137)
            out_dx = out_dx + p.gcat[((long)b * 12 + 9) * HW + pix] * p.inv_div_flow;
            out_dy = out_dy + p.gcat[((long)b * 12 + 10) * HW + pix] * p.inv_div_flow;
        }
        store_out(p.gflow + (long)b * 2 * HW + pix, out_dx);
        store_out(p.gflow + (long)b * 2 * HW + HW + pix, out_dy);
    }
    if ((p.abl & 8) && p.dbg && tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's atomics and stores have left the CU's queue
        stamp(5);
        unsigned long long *d = p.dbg + (long)blockIdx.x * 8;
        for (int i = 0; i < 6; ++i) d[i] = ts[i];
        d[6] = (unsigned long long)xcd_remap(blockIdx.x, gridDim.x);   // the tile this workgroup took
    }
}

// Row N2's backward for shapes the tiled kernel does not take (any C, any size): one lane per pixel, corners from global memory,
// 4 atomics per (pixel, channel) onto a gradient the host initialised with the concat gradient's slice.
template <bool DET = false>   // DET: as resample_bwd_kernel (planes b * C + c of H x W cells: the second image's gradient)
__global__ __launch_bounds__(256) void warp_diff_norm_cat_bwd_kernel(const float *__restrict__ pair, const float *__restrict__ flow,
                                                                     const float *__restrict__ outcat, const float *__restrict__ gcat,
                                                                     float *__restrict__ gpair, float *__restrict__ gflow,
                                                                     int C, int H, int W, long npix, float inv_div_flow, int norm_only, int bilinear,
                                                                     DetAcc det = DetAcc{})
{
    // norm_only (models.py:157-161 differentiated): outcat / gcat are the B x 1 x H x W norm and its gradient; the warped image is not
    // stored and is recomputed with the forward's arithmetic; no concat terms
    const long HW = (long)H * W;
    const int CC = 3 * C + 3;
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < npix; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % W);
        const long row = g / W;
        const int y = (int)(row % H), b = (int)(row / H);
        const long pix = (long)y * W + x;
        // position, sample and flow gradient written out: each shared helper (resample2d_common.h) changes this kernel's code
        const float xf = (float)x + flow[(long)b * 2 * HW + pix], yf = (float)y + flow[(long)b * 2 * HW + HW + pix];
        const float fx = floorf(xf), fy = floorf(yf);
        const int ixL = f2i_sat(fx), ixR = f2i_sat(fx + 1.0f), iyT = f2i_sat(fy), iyB = f2i_sat(fy + 1.0f);
        const int xL = clampi(ixL, 0, W - 1), xR = clampi(ixR, 0, W - 1), yT = clampi(iyT, 0, H - 1), yB = clampi(iyB, 0, H - 1);
        const float gam_y = 1 - (xf - fx), gam_x = 1 - (yf - fy);
        const float alpha = xf - (float)f2i_sat(xf), beta = yf - (float)f2i_sat(yf);
        const float s00 = (1 - alpha) * (1 - beta), s01 = alpha * (1 - beta), s10 = (1 - alpha) * beta, s11 = alpha * beta;
        const float gn = norm_only ? gcat[(long)b * HW + pix] : gcat[((long)b * CC + 3 * C + 2) * HW + pix];
        const float nrm = norm_only ? outcat[(long)b * HW + pix] : outcat[((long)b * CC + 3 * C + 2) * HW + pix];
        float out_dx = 0.0f, out_dy = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float *I = pair + ((long)b * 2 * C + C + c) * HW;
            float warped;
            if (!norm_only) warped = outcat[((long)b * CC + 2 * C + c) * HW + pix];
            else if (bilinear) {
                const double a = (double)(xf - fx), be = (double)(yf - fy);
                warped = 0.0f;
                warped = warped + (float)(((1. - a) * (1. - be)) * (double)I[yT * W + xL]);
                warped = warped + (float)((a * (1. - be)) * (double)I[yT * W + xR]);
                warped = warped + (float)(((1. - a) * be) * (double)I[yB * W + xL]);
                warped = warped + (float)((a * be) * (double)I[yB * W + xR]);
            } else {
                const int xN = clampi(d2i_sat(floor((double)xf + 0.5)), 0, W - 1), yN = clampi(d2i_sat(floor((double)yf + 0.5)), 0, H - 1);
                warped = I[yN * W + xN];
            }
            const float diff = pair[((long)b * 2 * C + c) * HW + pix] - warped;
            const float gd = chnorm_grad(gn, diff, nrm);
            const float go = norm_only ? 0.0f - gd : gcat[((long)b * CC + 2 * C + c) * HW + pix] - gd;
            if (gpair) {
                gpair[((long)b * 2 * C + c) * HW + pix] = gcat[((long)b * CC + c) * HW + pix] + gd;
                if constexpr (DET) {
                    int ds;
                    if (det_scale(det.pmax[(long)b * C + c], det.K, ds)) {
                        unsigned long long *A = det.acc + ((long)b * C + c) * HW;
                        det_add(A + yT * W + xL, s00 * go, ds);
                        det_add(A + yT * W + xR, s01 * go, ds);
                        det_add(A + yB * W + xL, s10 * go, ds);
                        det_add(A + yB * W + xR, s11 * go, ds);
                    }
                } else {
                    float *G = gpair + ((long)b * 2 * C + C + c) * HW;
                    unsafeAtomicAdd(G + yT * W + xL, s00 * go);
                    unsafeAtomicAdd(G + yT * W + xR, s01 * go);
                    unsafeAtomicAdd(G + yB * W + xL, s10 * go);
                    unsafeAtomicAdd(G + yB * W + xR, s11 * go);
                }
            }
            const float iTL = I[yT * W + xL], iTR = I[yT * W + xR], iBL = I[yB * W + xL], iBR = I[yB * W + xR];
            out_dy = out_dy + (gam_y * go) * iBL;
            out_dy = out_dy - (gam_y * go) * iTL;
            out_dy = out_dy + ((1 - gam_y) * go) * iBR;
            out_dy = out_dy - ((1 - gam_y) * go) * iTR;
            out_dx = out_dx + (gam_x * go) * iTR;
            out_dx = out_dx - (gam_x * go) * iTL;
            out_dx = out_dx + ((1 - gam_x) * go) * iBR;
            out_dx = out_dx - ((1 - gam_x) * go) * iBL;
        }
        if (norm_only) { gflow[(long)b * 2 * HW + pix] = out_dx; gflow[(long)b * 2 * HW + HW + pix] = out_dy; continue; }
        gflow[(long)b * 2 * HW + pix] = out_dx + gcat[((long)b * CC + 3 * C) * HW + pix] * inv_div_flow;
        gflow[(long)b * 2 * HW + HW + pix] = out_dy + gcat[((long)b * CC + 3 * C + 1) * HW + pix] * inv_div_flow;
    }
}

// ---------------------------------------------------------------- deterministic grad_input1: prepass, fallback, conversion
// MODE 0: the scattered gradient is grad_out (B x C x H x W); MODE 1: it is warp_diff_norm_cat's g_warped, formed from the concat gradient
// with the fused kernels' arithmetic (warp_diff_norm_cat_bwd_kernel, c3x_load_go).
struct DetSrc {
    const float *gout;                          // MODE 0
    const float *gcat, *pair, *outcat;          // MODE 1
    int C;
    long HW;
};
template <int MODE>
__device__ __forceinline__ float det_src(const DetSrc &d, int b, int c, long pix)
{
    if constexpr (MODE == 0) return d.gout[((long)b * d.C + c) * d.HW + pix];
    const long CC = 3L * d.C + 3;
    const float gn = d.gcat[((long)b * CC + 3 * d.C + 2) * d.HW + pix], nrm = d.outcat[((long)b * CC + 3 * d.C + 2) * d.HW + pix];
    const float diff = d.pair[((long)b * 2 * d.C + c) * d.HW + pix] - d.outcat[((long)b * CC + 2 * d.C + c) * d.HW + pix];
    return d.gcat[((long)b * CC + 2 * d.C + c) * d.HW + pix] - chnorm_grad(gn, diff, nrm);
}

// max |g| per plane as the bits of |g| (their integer order is the order of the magnitudes, NaN above inf): one integer atomicMax per
// workgroup, whatever order the workgroups arrive in.  A workgroup takes DET_MAX_PER x 256 consecutive values of one plane, its loads all
// in flight at once.  Grid: planes x chunks, chunk = blockIdx.x % chunks.
constexpr int DET_MAX_PER = 16;
template <int MODE>
__global__ __launch_bounds__(256) void det_plane_max_kernel(const DetSrc d, unsigned *__restrict__ pmax, int chunks)
{
    __shared__ unsigned wmax[4];
    const long plane = blockIdx.x / chunks;
    const int b = (int)(plane / d.C), c = (int)(plane % d.C);
    const long i0 = (long)(blockIdx.x % chunks) * (256L * DET_MAX_PER) + threadIdx.x;
    float v[DET_MAX_PER];
    if ((long)(blockIdx.x % chunks + 1) * (256L * DET_MAX_PER) <= d.HW) {   // a whole chunk: unconditional loads, all issued before any use
#pragma unroll
        for (int j = 0; j < DET_MAX_PER; ++j) v[j] = det_src<MODE>(d, b, c, i0 + 256L * j);
    } else {
#pragma unroll
        for (int j = 0; j < DET_MAX_PER; ++j) v[j] = i0 + 256L * j < d.HW ? det_src<MODE>(d, b, c, i0 + 256L * j) : 0.0f;
    }
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < DET_MAX_PER; ++j) m = max(m, __float_as_uint(v[j]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        if (m != 0u) atomicMax(pmax + plane, m);
    }
}

// Planes with an inf or a NaN: the oracle's serial fp32 scatter (y, x, window offsets, corners TL TR BL BR) straight into the
// gradient, one lane per plane (lanes of finite planes return at once).  `G0`: plane (b, c) starts at G0 + b * g_bs + c * Hi * Wi.
template <int MODE>
__device__ void det_fallback(const DetSrc &d, const float *__restrict__ flow, const unsigned *__restrict__ pmax, float *__restrict__ G0,
                             long g_bs, int B, int Hi, int Wi, int H, int W, int ks, long plane)
{
    if (plane >= (long)B * d.C || pmax[plane] < 0x7f800000u) return;
    const int b = (int)(plane / d.C), c = (int)(plane % d.C);
    const long HW = (long)H * W;
    float *G = G0 + (long)b * g_bs + (long)c * Hi * Wi;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const long p = (long)y * W + x;
            // written out: warp_bwd_pos converts in another order, which changes this kernel's branches
            const float xf = (float)x + flow[(long)b * 2 * HW + p], yf = (float)y + flow[(long)b * 2 * HW + HW + p];
            const float alpha = xf - (float)f2i_sat(xf), beta = yf - (float)f2i_sat(yf);
            const float fx = floorf(xf), fy = floorf(yf);
            const int xL = clampi(f2i_sat(fx), 0, Wi - 1), xR = clampi(f2i_sat(fx + 1.0f), 0, Wi - 1);
            const int yT = clampi(f2i_sat(fy), 0, Hi - 1), yB = clampi(f2i_sat(fy + 1.0f), 0, Hi - 1);
            const float go = det_src<MODE>(d, b, c, p);
            const float s00 = (1 - alpha) * (1 - beta), s01 = alpha * (1 - beta), s10 = (1 - alpha) * beta, s11 = alpha * beta;
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx) {
                    const long yt = (long)clampi(yT + ky, 0, Hi - 1) * Wi, yb = (long)clampi(yB + ky, 0, Hi - 1) * Wi;
                    const int xl = clampi(xL + kx, 0, Wi - 1), xr = clampi(xR + kx, 0, Wi - 1);
                    G[yt + xl] = G[yt + xl] + s00 * go;
                    G[yt + xr] = G[yt + xr] + s01 * go;
                    G[yb + xl] = G[yb + xl] + s10 * go;
                    G[yb + xr] = G[yb + xr] + s11 * go;
                }
        }
}

// Step 5 of the contract: r = (float)((double)Q * 2^-s) -- int64 -> double and double -> float, both round-to-nearest-even, subnormals
// kept -- and one fp32 add into the gradient.  Planes that add nothing (all zero, or non-finite) are left untouched here: the last
// `gridDim.x - ncvt` workgroups run the serial fallback of the non-finite ones, one lane per plane (disjoint cells, no ordering needed).
template <int MODE>
__global__ __launch_bounds__(256) void det_convert_kernel(const unsigned long long *__restrict__ acc, const unsigned *__restrict__ pmax, int K,
                                                          float *__restrict__ G0, long g_bs, int C, long HWi, long ncell, unsigned ncvt,
                                                          const DetSrc d, const float *__restrict__ flow, int B, int Hi, int Wi, int H, int W,
                                                          int ks)
{
    if (blockIdx.x >= ncvt) {
        det_fallback<MODE>(d, flow, pmax, G0, g_bs, B, Hi, Wi, H, W, ks, (long)(blockIdx.x - ncvt) * blockDim.x + threadIdx.x);
        return;
    }
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < ncell; i += (long)ncvt * blockDim.x) {
        const long plane = i / HWi, cell = i - plane * HWi;
        int s;
        if (!det_scale(pmax[plane], K, s)) continue;
        const float r = __double2float_rn(ldexp(__ll2double_rn((long long)acc[i]), -s));
        float *g = G0 + (plane / C) * g_bs + (plane % C) * HWi + cell;
        *g = *g + r;
    }
}

// N2 for shapes the tiled kernel does not take: one lane per pixel, corners gathered from global memory.
__global__ __launch_bounds__(256) void warp_diff_norm_cat_kernel(const float *__restrict__ pair, const float *__restrict__ flow,
                                                                 float *__restrict__ out, int C, int H, int W, long npix,
                                                                 int bilinear, float div_flow, int norm_only)
{
    const long HW = (long)H * W;
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < npix; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % W);
        const long row = g / W;
        const int y = (int)(row % H), b = (int)(row / H);
        const long pix = (long)y * W + x;
        const float dx = flow[(long)b * 2 * HW + pix], dy = flow[(long)b * 2 * HW + HW + pix];
        const float xf = (float)x + dx, yf = (float)y + dy;
        int xL, xR, yT, yB;   // one clamp (the image has the flow's size), written out: warp_pos / warp_fwd_corners change this kernel's code
        float alpha = 0.0f, beta = 0.0f;
        if (bilinear) {
            const float fx = floorf(xf), fy = floorf(yf);
            alpha = xf - fx; beta = yf - fy;
            xL = clampi(f2i_sat(fx), 0, W - 1); xR = clampi(f2i_sat(fx + 1.0f), 0, W - 1);
            yT = clampi(f2i_sat(fy), 0, H - 1); yB = clampi(f2i_sat(fy + 1.0f), 0, H - 1);
        } else {
            xL = xR = clampi(d2i_sat(floor((double)xf + 0.5)), 0, W - 1);
            yT = yB = clampi(d2i_sat(floor((double)yf + 0.5)), 0, H - 1);
        }
        const BilinearW w = bilinear_weights(alpha, beta);
        float *ob = out + (long)b * (3 * C + 3) * HW + pix;
        float ssq = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float *I = pair + ((long)b * 2 * C + C + c) * HW;
            float val;
            if (bilinear) val = bilinear_sample(w, I[(long)yT * W + xL], I[(long)yT * W + xR], I[(long)yB * W + xL], I[(long)yB * W + xR]);
            else val = I[(long)yT * W + xL];
            const float v0 = pair[((long)b * 2 * C + c) * HW + pix];
            if (!norm_only) {
                ob[(long)c * HW] = v0;
                ob[(long)(C + c) * HW] = I[pix];
                ob[(long)(2 * C + c) * HW] = val;
            }
            const float d = v0 - val;
            ssq = ssq + d * d;
        }
        if (norm_only) { out[(long)b * HW + pix] = sqrtf(ssq); continue; }
        const float inv_div = 1.0f / div_flow;   // as PyTorch divides a GPU tensor by a scalar
        ob[(long)(3 * C) * HW] = dx * inv_div;
        ob[(long)(3 * C + 1) * HW] = dy * inv_div;
        ob[(long)(3 * C + 2) * HW] = sqrtf(ssq);
    }
}

// Tile height of the tiled kernels (two 1024-thread workgroups per CU = 512 resident tiles): the height that needs fewer
// window rows over all rounds; 48 turns FlowNet2's 8 x 384 x 512 into exactly one round.
static inline int tile_height(int B, int H, int tiles_x)
{
    const long slots = 512;
    const long t32 = (long)B * tiles_x * ((H + 31) / 32), t48 = (long)B * tiles_x * ((H + 47) / 48);
    const long c32 = ((t32 + slots - 1) / slots) * (32 + 32), c48 = ((t48 + slots - 1) / slots) * (48 + 32);
    return c48 < c32 ? 48 : 32;
}

} // namespace fn2

// ---------------------------------------------------------------- host side: checks, strides, launches
using namespace fn2;

// The checks come in the same order in every entry point: dims (with kernel_size / div_flow) -> FN2_EINVAL, empty -> FN2_OK,
// null -> FN2_EINVAL, (det) workspace -> FN2_EINVAL, alignment -> FN2_EALIGN.
static bool resample_dims_bad(int B, int C, int Hi, int Wi, int H, int W, int kernel_size)
{
    return B < 0 || C < 0 || Hi < 1 || Wi < 1 || H < 0 || W < 0 || kernel_size < 1;
}
static bool pair_dims_bad(int B, int C, int H, int W, float div_flow = 1.0f)
{
    return B < 0 || C < 1 || H < 1 || W < 1 || !(div_flow == div_flow) || div_flow == 0.0f;
}
template <class... P> static bool any_null(P... p) { return (... || (p == nullptr)); }
template <class... P> static bool all_aligned(size_t bytes, P... p) { return (... && aligned(p, bytes)); }

// the caller's strides, or those of a dense B x C x Hi x Wi image
static ImgStrides dense_or(const int64_t *st, int C, int Hi, int Wi)
{
    if (st) return ImgStrides{st[0], st[1], st[2], st[3]};
    return ImgStrides{(long)C * Hi * Wi, (long)Hi * Wi, Wi, 1};
}
// the second image of a dense B x 2C x H x W pair (the one that is warped) and its strides
static const float *pair_second(const float *pair, int C, int H, int W, ImgStrides &is)
{
    const long HW = (long)H * W;
    is = ImgStrides{2L * C * HW, HW, W, 1};
    return pair + (long)C * HW;
}
// shapes the LDS-window kernels take: image rows contiguous and 16 B aligned, same size as the flow, large enough to tile
static bool tiled_shape_ok(const ImgStrides &is, const float *img, int Hi, int Wi, int H, int W)
{
    return (is.w == 1) && (is.h % 4 == 0) && (is.c % 4 == 0) && (is.b % 4 == 0) && aligned(img, 16) && (Hi == H) && (Wi == W) &&
           (W % 4 == 0) && (H >= 16) && (W >= 32);
}
static dim3 tile_grid(int B, int tiles_x, int tiles_y) { return dim3((unsigned)((long)B * tiles_x * tiles_y)); }

// resample_fwd_tiled<TH, 64, 16, FUSE> on a tiled shape (image of the flow's size), TH = 32 or 48: `th`, or tile_height's choice
template <int FUSE>
static void launch_fwd_tiled(const float *img, const ImgStrides &is, const float *flow, float *out, int B, int C, int H, int W, int bilinear,
                             const float *pair, float div_flow, hipStream_t s, int th = 0)
{
    const int tiles_x = (W + 63) / 64;
    if (!th) th = tile_height(B, H, tiles_x);
    const int tiles_y = (H + th - 1) / th;
    if (th == 48)
        hipLaunchKernelGGL((resample_fwd_tiled<48, 64, 16, FUSE>), tile_grid(B, tiles_x, tiles_y), dim3(1024), 0, s, img, is, flow, out, C, H,
                           W, H, W, tiles_x, tiles_y, bilinear, pair, div_flow);
    else
        hipLaunchKernelGGL((resample_fwd_tiled<32, 64, 16, FUSE>), tile_grid(B, tiles_x, tiles_y), dim3(1024), 0, s, img, is, flow, out, C, H,
                           W, H, W, tiles_x, tiles_y, bilinear, pair, div_flow);
}

// argument block of resample_bwd_c3x for 32 x 64 tiles (the fields of the fused form are set by its caller)
static C3xArgs c3x_args(const float *img, ImgStrides is, const float *flow, float *gimg, long gimg_bs, float *gflow, int B, int Hi, int Wi,
                        int H, int W, int abl)
{
    C3xArgs a;
    a.img = img; a.is = is; a.flow = flow; a.gout = nullptr; a.gcat = a.pair = a.outcat = nullptr; a.gpair0 = nullptr;
    a.gimg = gimg; a.gimg_bs = gimg_bs; a.gflow = gflow;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.H = H; a.W = W; a.tiles_x = (W + 63) / 64; a.tiles_y = (H + 31) / 32; a.abl = abl;
    a.inv_div_flow = 0.0f; a.bilinear = 1;
#ifdef FN2_DEBUG_BUILD
    a.dbg = static_cast<unsigned long long *>(corr_f16x2_get_debug_buffer());
#else
    a.dbg = nullptr;
#endif
    return a;
}
template <int FUSED, bool SCATTER> static void launch_c3x(const C3xArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL((resample_bwd_c3x<32, 64, 16, 1024, FUSED, SCATTER>), tile_grid(a.B, a.tiles_x, a.tiles_y), dim3(1024), 0, s, a);
}

// grad_pair[:, C:] = grad_cat[:, C:2C]: the second image's gradient starts as its slice of the concat gradient (one strided copy), then
// the scatter adds
static hipError_t seed_second_grad(float *grad_pair, const float *grad_cat, int B, int C, long HW, hipStream_t s)
{
    return hipMemcpy2DAsync(grad_pair + (long)C * HW, 2 * C * HW * sizeof(float), grad_cat + (long)C * HW, (3 * C + 3) * HW * sizeof(float),
                            C * HW * sizeof(float), B, hipMemcpyDeviceToDevice, s);
}

// `bilinear` of the two impl functions: bit 0 = bilinear (else nearest; both reference backward kernels ignore it); the
// bits from 8 up are profiling switches that only fn2_debug_resample2d_* set (0 from the public entry points and the bindings).  The
// values are the ones the scripts pass (scripts/resample_micro.py, resample_r5_micro.py, resample_timeline.py).
enum : int {
    RS_BILINEAR = 1,
    RS_UNTILED = 0x100,    // bit 8: the untiled kernels
    RS_ABL_SHIFT = 9,      // bits 9-11: the backward kernels' ablations (`abl` bits 0-2: no flush, no scatter, no gather)
    RS_TILE_SHIFT = 12,    // bits 12-13: tile height, 0 = automatic (1 = 48, 2 = 32, 3 = 96 with every channel resident forward, 64 backward)
    RS_FORM_SHIFT = 14,    // bits 14-15, forward: 4 adjacent pixels per thread (1 = 48 x 64 tiles, 2 = 64 x 64); backward: accumulation window
                           // (1 = fp64 cells 48 x 64 +- 12, 2 = fp64 cells 32 x 64 +- 16, 3 = fp64 cells 48 x 64 +- 16, one workgroup per CU)
    RS_STAMPS = 0x10000,   // bit 16: wall-clock stamps into the debug buffer (`abl` bit 3)
};
static int rs_tile(int f) { return (f >> RS_TILE_SHIFT) & 3; }
static int rs_form(int f) { return (f >> RS_FORM_SHIFT) & 3; }
static int rs_variant(int f) { return (f >> RS_TILE_SHIFT) & 15; }   // tile and form bits together: the backward's selector
static int rs_abl(int f) { return ((f >> RS_ABL_SHIFT) & 7) | ((f & RS_STAMPS) ? 8 : 0); }

static int resample2d_forward_impl(const float *img, const int64_t *img_strides, const float *flow, float *out,
                                   int B, int C, int Hi, int Wi, int H, int W,
                                   int kernel_size, int bilinear, void *stream)
{
    if (resample_dims_bad(B, C, Hi, Wi, H, W, kernel_size)) return FN2_EINVAL;
    if ((long)B * C * H * W == 0) return FN2_OK;
    if (any_null(img, flow, out)) return FN2_EINVAL;
    if (!all_aligned(4, img, flow, out)) return FN2_EALIGN;
    const ImgStrides is = dense_or(img_strides, C, Hi, Wi);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long npix = (long)B * H * W;
    const int bil = bilinear & RS_BILINEAR;
    if (kernel_size != 1) {
        hipLaunchKernelGGL(resample_fwd_ks_kernel, dim3(stream_grid(npix)), dim3(256), 0, s, img, is, flow, out, C, Hi, Wi, H, W,
                           npix, kernel_size, bil);
    } else if (tiled_shape_ok(is, img, Hi, Wi, H, W) && !(bilinear & RS_UNTILED)) {
        const int tiles_x = (W + 63) / 64, px4 = all_aligned(16, flow, out) ? rs_form(bilinear) : 0;
        if (px4 == 1) {          // profiling: 4 adjacent pixels per thread, 48 x 64 tiles
            const int tiles_y = (H + 47) / 48;
            hipLaunchKernelGGL((resample_fwd_tiled4<48, 16>), tile_grid(B, tiles_x, tiles_y), dim3(768), 0, s, img, is, flow, out, C, Hi, Wi,
                               H, W, tiles_x, tiles_y, bil);
        } else if (px4 == 2) {   // ... 64 x 64 tiles, 1024 threads
            const int tiles_y = (H + 63) / 64;
            hipLaunchKernelGGL((resample_fwd_tiled4<64, 16>), tile_grid(B, tiles_x, tiles_y), dim3(1024), 0, s, img, is, flow, out, C, Hi, Wi,
                               H, W, tiles_x, tiles_y, bil);
        } else if (rs_tile(bilinear) == 3 && C == 3) {   // profiling: every channel window resident, 96 x 64 tiles, one workgroup per CU
            const int tiles_y = (H + 95) / 96;
            hipLaunchKernelGGL((resample_fwd_tiled_all<96, 64, 16, 3>), tile_grid(B, tiles_x, tiles_y), dim3(1024), 0, s, img, is, flow, out,
                               Hi, Wi, H, W, tiles_x, tiles_y, bil);
        } else if (rs_variant(bilinear) == 0 && C == 3) {
            // C == 3 (FlowNet2's only use): the three channel windows resident at once in 32 x 64 tiles (73.7 KB: two workgroups per
            // CU), one barrier in the whole kernel, corner offsets and weights formed once per pixel -- 8 x 3 x 384 x 512: 19.3 us
            // against 20.9 for the per-channel kernel (smooth flow 18.1 / 19.1), same bits
            const int tiles_y = (H + 31) / 32;
            unsigned long long *dbgbuf = nullptr;
#ifdef FN2_DEBUG_BUILD
            if (bilinear & RS_STAMPS) dbgbuf = static_cast<unsigned long long *>(corr_f16x2_get_debug_buffer());   // profiling: timeline stamps
#endif
            // (512 persistent workgroups taking one tile and then half of one of the remaining 256 -- one balanced round instead of one
            // and a half -- measured slower: 18.6 us against 17.0, the half tile costs 4.8 us of fixed latencies)
            hipLaunchKernelGGL((resample_fwd_tiled_all<32, 64, 16, 3, 8>), tile_grid(B, tiles_x, tiles_y), dim3(1024), 0, s, img, is, flow,
                               out, Hi, Wi, H, W, tiles_x, tiles_y, bil, dbgbuf);
        } else {
            const int th = rs_tile(bilinear) ? (rs_tile(bilinear) == 1 ? 48 : 32) : 0;   // profiling: a forced tile height
            launch_fwd_tiled<0>(img, is, flow, out, B, C, H, W, bil, nullptr, 1.0f, s, th);
        }
    } else if (W % 4 == 0 && all_aligned(16, flow, out)) {
        const long ng = npix / 4;
        hipLaunchKernelGGL(resample_fwd_kernel<4>, dim3(stream_grid(ng)), dim3(256), 0, s, img, is, flow, out, C, Hi, Wi, H, W, ng, bil);
    } else {
        hipLaunchKernelGGL(resample_fwd_kernel<1>, dim3(stream_grid(npix)), dim3(256), 0, s, img, is, flow, out, C, Hi, Wi, H, W, npix, bil);
    }
    return launch_status();
}

extern "C" int fn2_resample2d_forward(const float *img, const int64_t *img_strides, const float *flow, float *out,
                                      int B, int C, int Hi, int Wi, int H, int W,
                                      int kernel_size, int bilinear, void *stream)
{
    return resample2d_forward_impl(img, img_strides, flow, out, B, C, Hi, Wi, H, W, kernel_size, bilinear != 0 ? 1 : 0, stream);
}

#ifdef FN2_DEBUG_BUILD
extern "C" int fn2_debug_resample2d_forward(const float *img, const int64_t *img_strides, const float *flow, float *out,
                                            int B, int C, int Hi, int Wi, int H, int W,
                                            int kernel_size, int bilinear, int flags, void *stream)
{
    return resample2d_forward_impl(img, img_strides, flow, out, B, C, Hi, Wi, H, W, kernel_size,
                                   (bilinear != 0 ? 1 : 0) | (flags & ~0xff), stream);
}
#endif

static int resample2d_backward_impl(const float *img, const int64_t *img_strides, const float *flow,
                                    const float *grad_out, float *grad_img, float *grad_flow,
                                    int B, int C, int Hi, int Wi, int H, int W,
                                    int kernel_size, int bilinear, void *stream)
{
    if (resample_dims_bad(B, C, Hi, Wi, H, W, kernel_size)) return FN2_EINVAL;
    if ((long)B * H * W == 0) return FN2_OK;
    if (any_null(img, flow, grad_out, grad_img, grad_flow)) return FN2_EINVAL;
    if (!all_aligned(4, img, flow, grad_out, grad_img, grad_flow)) return FN2_EALIGN;
    const ImgStrides is = dense_or(img_strides, C, Hi, Wi);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long npix = (long)B * H * W;
    if (kernel_size != 1) {
        hipLaunchKernelGGL(resample_bwd_ks_kernel<false>, dim3(stream_grid(npix)), dim3(256), 0, s, img, is, flow, grad_out, grad_img,
                           grad_flow, C, Hi, Wi, H, W, npix, kernel_size);
    } else if (tiled_shape_ok(is, img, Hi, Wi, H, W) && !(bilinear & RS_UNTILED)) {
        const int abl = rs_abl(bilinear), tiles_x = (W + 63) / 64;
#define FN2_RB(TH, R, WPE, ACC)                                                                                        \
    do {                                                                                                               \
        const int tiles_y = (H + TH - 1) / TH;                                                                         \
        hipLaunchKernelGGL((resample_bwd_tiled<TH, 64, R, 1024, WPE, ACC>), tile_grid(B, tiles_x, tiles_y), dim3(1024), 0, s, img, is, \
                           flow, grad_out, grad_img, grad_flow, C, Hi, Wi, H, W, tiles_x, tiles_y, abl);               \
    } while (0)
        switch (rs_variant(bilinear)) {   // profiling: tile height and accumulation window (the table above)
        case 1: FN2_RB(48, 16, 8, 0); break;
        case 2: FN2_RB(32, 16, 8, 0); break;
        case 3: FN2_RB(64, 16, 8, 0); break;
        case 4: FN2_RB(48, 12, 8, 1); break;
        case 8: FN2_RB(32, 16, 8, 1); break;
        case 12: FN2_RB(48, 16, 4, 1); break;
        case 5: FN2_RB(48, 12, 8, 0); break;
        case 6: FN2_RB(96, 16, 4, 0); break;
        case 7: FN2_RB(96, 16, 4, 1); break;
        case 9: FN2_RB(48, 16, 4, 0); break;
        case 10: if (tile_height(B, H, tiles_x) == 48) FN2_RB(48, 16, 8, 0); else FN2_RB(32, 16, 8, 0); break;   // the round-3 choice
        // C == 3 (FlowNet2's only use): the three channels in one scatter, workgroup order alternating with i / 8 -- 8 x 3 x 384 x 512,
        // white-noise flow 51.0 us, smooth flow 37.7.  Other C: one channel at a time, 32-row tiles with fp64 cells (74 KB of LDS, two
        // workgroups per CU; selector 8): 54.2 / 38.6 us against 57.2-59.8 / 44.5 for the 48 x 64 fp32 tiles of round 3 (selector 10)
        default:
            if (C == 3) {
                C3xArgs a = c3x_args(img, is, flow, grad_img, (long)C * Hi * Wi, grad_flow, B, Hi, Wi, H, W, abl);
                a.gout = grad_out;
                launch_c3x<0, true>(a, s);
            } else FN2_RB(32, 16, 8, 1);
            break;
        }
#undef FN2_RB
    } else {
        hipLaunchKernelGGL(resample_bwd_kernel<false>, dim3(stream_grid(npix)), dim3(256), 0, s, img, is, flow, grad_out,
                           grad_img, grad_flow, C, Hi, Wi, H, W, npix);
    }
    return launch_status();
}

extern "C" int fn2_resample2d_backward(const float *img, const int64_t *img_strides, const float *flow,
                                       const float *grad_out, float *grad_img, float *grad_flow,
                                       int B, int C, int Hi, int Wi, int H, int W,
                                       int kernel_size, int bilinear, void *stream)
{
    return resample2d_backward_impl(img, img_strides, flow, grad_out, grad_img, grad_flow, B, C, Hi, Wi, H, W, kernel_size,
                                    bilinear != 0 ? 1 : 0, stream);
}

#ifdef FN2_DEBUG_BUILD
extern "C" int fn2_debug_resample2d_backward(const float *img, const int64_t *img_strides, const float *flow,
                                             const float *grad_out, float *grad_img, float *grad_flow,
                                             int B, int C, int Hi, int Wi, int H, int W,
                                             int kernel_size, int bilinear, int flags, void *stream)
{
    return resample2d_backward_impl(img, img_strides, flow, grad_out, grad_img, grad_flow, B, C, Hi, Wi, H, W, kernel_size,
                                    (bilinear != 0 ? 1 : 0) | (flags & ~0xff), stream);
}
#endif

// Row N2 (fn2_warp_diff_norm_cat) and its norm-only form (fn2_warp_diff_norm, models.py:157-161 / :170-174:
// ||pair[:, :C] - Resample2d(pair[:, C:], flow)||_2 with no concat -- the same kernels storing only the norm plane)
template <int FUSE>   // 1: the concat; 2: the norm plane only
static int warp_diff_norm_forward(const float *pair, const float *flow, float *out, float div_flow, int B, int C, int H, int W, int bilinear,
                                  void *stream)
{
    bilinear = bilinear != 0 ? 1 : 0;
    if (pair_dims_bad(B, C, H, W, div_flow)) return FN2_EINVAL;
    if ((long)B * H * W == 0) return FN2_OK;
    if (any_null(pair, flow, out)) return FN2_EINVAL;
    if (!all_aligned(4, pair, flow, out)) return FN2_EALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ImgStrides is;
    const float *img1 = pair_second(pair, C, H, W, is);
    if (tiled_shape_ok(is, img1, H, W, H, W)) {
        launch_fwd_tiled<FUSE>(img1, is, flow, out, B, C, H, W, bilinear, pair, div_flow, s);
    } else {
        const long npix = (long)B * H * W;
        hipLaunchKernelGGL(warp_diff_norm_cat_kernel, dim3(stream_grid(npix)), dim3(256), 0, s, pair, flow, out, C, H, W, npix, bilinear,
                           div_flow, FUSE == 2 ? 1 : 0);
    }
    return launch_status();
}

extern "C" int fn2_warp_diff_norm_cat(const float *pair, const float *flow, float *out, float div_flow,
                                      int B, int C, int H, int W, int bilinear, void *stream)
{
    return warp_diff_norm_forward<1>(pair, flow, out, div_flow, B, C, H, W, bilinear, stream);
}

extern "C" int fn2_warp_diff_norm(const float *pair, const float *flow, float *out_norm, int B, int C, int H, int W, int bilinear, void *stream)
{
    return warp_diff_norm_forward<2>(pair, flow, out_norm, 1.0f, B, C, H, W, bilinear, stream);
}

extern "C" int fn2_warp_diff_norm_cat_backward(const float *pair, const float *flow, const float *out_cat, const float *grad_cat,
                                               float *grad_pair, float *grad_flow, float div_flow, int B, int C, int H, int W,
                                               int bilinear, void *stream)
{
    (void)bilinear;   // both reference backward kernels ignore the flag (resample2d_kernel.cu:75-198)
    if (pair_dims_bad(B, C, H, W, div_flow)) return FN2_EINVAL;
    if ((long)B * H * W == 0) return FN2_OK;
    if (any_null(pair, flow, out_cat, grad_cat, grad_flow)) return FN2_EINVAL;
    if (!all_aligned(4, pair, flow, out_cat, grad_cat, grad_flow, grad_pair)) return FN2_EALIGN;   // grad_pair may be null
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long HW = (long)H * W, npix = (long)B * HW;
    const float inv = 1.0f / div_flow;
    if (grad_pair) {
        hipError_t e = seed_second_grad(grad_pair, grad_cat, B, C, HW, s);
        if (e != hipSuccess) return (int)e;
    }
    ImgStrides is;
    const float *img1 = pair_second(pair, C, H, W, is);
    if (C == 3 && tiled_shape_ok(is, img1, H, W, H, W)) {
        C3xArgs a = c3x_args(img1, is, flow, grad_pair ? grad_pair + 3 * HW : nullptr, 6 * HW, grad_flow, B, H, W, H, W, 0);
        a.gcat = grad_cat; a.pair = pair; a.outcat = out_cat; a.gpair0 = grad_pair; a.inv_div_flow = inv;
        if (grad_pair) launch_c3x<1, true>(a, s);
        else launch_c3x<1, false>(a, s);
    } else {
        hipLaunchKernelGGL(warp_diff_norm_cat_bwd_kernel<false>, dim3(stream_grid(npix)), dim3(256), 0, s, pair, flow, out_cat, grad_cat,
                           grad_pair, grad_flow, C, H, W, npix, inv, 0, 1);
    }
    return launch_status();
}

// fn2_warp_diff_norm's backward with respect to the flow (the pair is the network's input in FlowNet2; compose the unfused entry points
// when it needs a gradient): grad_flow = Resample2d's flow gradient for g_warped = -grad_norm * diff / (norm + 1e-9), the warp recomputed
extern "C" int fn2_warp_diff_norm_backward(const float *pair, const float *flow, const float *norm, const float *grad_norm,
                                           float *grad_flow, int B, int C, int H, int W, int bilinear, void *stream)
{
    bilinear = bilinear != 0 ? 1 : 0;
    if (pair_dims_bad(B, C, H, W)) return FN2_EINVAL;
    if ((long)B * H * W == 0) return FN2_OK;
    if (any_null(pair, flow, norm, grad_norm, grad_flow)) return FN2_EINVAL;
    if (!all_aligned(4, pair, flow, norm, grad_norm, grad_flow)) return FN2_EALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ImgStrides is;
    const float *img1 = pair_second(pair, C, H, W, is);
    if (C == 3 && tiled_shape_ok(is, img1, H, W, H, W)) {
        C3xArgs a = c3x_args(img1, is, flow, nullptr, 0, grad_flow, B, H, W, H, W, 0);
        a.gcat = grad_norm; a.pair = pair; a.outcat = norm; a.bilinear = bilinear;
        launch_c3x<2, false>(a, s);
    } else {
        const long npix = (long)B * H * W;
        hipLaunchKernelGGL(warp_diff_norm_cat_bwd_kernel<false>, dim3(stream_grid(npix)), dim3(256), 0, s, pair, flow, norm, grad_norm,
                           static_cast<float *>(nullptr), grad_flow, C, H, W, npix, 0.0f, 1, bilinear);
    }
    return launch_status();
}

// ---------------------------------------------------------------- deterministic backward (fixed-point grad_input1)
// Workspace: the plane maxima (4 B per plane, rounded up to 256 B), then B*C planes of Hi x Wi int64 accumulators.
static size_t det_workspace_bytes(long planes, long HWi)
{
    return (size_t)((4 * planes + 255) / 256 * 256) + (size_t)(8 * planes * HWi);
}
// K of the contract: the smallest K with 2^K >= 16 k^2 H W
static int det_K(int ks, int H, int W)
{
    const unsigned long long n = 16ull * (unsigned long long)ks * ks * (unsigned long long)H * W;
    int K = 0;
    while (K < 63 && (1ull << K) < n) ++K;
    return K;
}

// clear the workspace and find the plane maxima (the first two steps of every deterministic call)
template <int MODE>
static int det_begin(const DetSrc &d, int B, void *workspace, size_t bytes, DetAcc &det, int K, hipStream_t s)
{
    const long planes = (long)B * d.C;
    const int rc = zero_fill_async(workspace, bytes, s);
    if (rc != FN2_OK) return rc;
    det.pmax = static_cast<unsigned *>(workspace);
    det.acc = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + (4 * planes + 255) / 256 * 256);
    det.K = K;
    if (planes > 0) {
        const int chunks = (int)((d.HW + 256L * DET_MAX_PER - 1) / (256L * DET_MAX_PER));
        hipLaunchKernelGGL(det_plane_max_kernel<MODE>, dim3((unsigned)(planes * chunks)), dim3(256), 0, s, d,
                           static_cast<unsigned *>(workspace), chunks);
    }
    return launch_status();
}

// the conversion of the finite planes and the serial scatter of the non-finite ones, in one launch
template <int MODE>
static void det_end(const DetSrc &d, const float *flow, const DetAcc &det, float *G0, long g_bs, int B, int Hi, int Wi, int H, int W, int ks,
                    hipStream_t s)
{
    const long planes = (long)B * d.C, HWi = (long)Hi * Wi;
    if (planes == 0) return;
    const unsigned ncvt = stream_grid(planes * HWi), nfb = (unsigned)((planes + 255) / 256);
    hipLaunchKernelGGL(det_convert_kernel<MODE>, dim3(ncvt + nfb), dim3(256), 0, s, det.acc, det.pmax, det.K, G0, g_bs, d.C, HWi, planes * HWi,
                       ncvt, d, flow, B, Hi, Wi, H, W, ks);
}

extern "C" size_t fn2_resample2d_backward_det_workspace_bytes(int B, int C, int Hi, int Wi, int H, int W, int kernel_size)
{
    if (resample_dims_bad(B, C, Hi, Wi, H, W, kernel_size)) return 0;
    return det_workspace_bytes((long)B * C, (long)Hi * Wi);
}

extern "C" int fn2_resample2d_backward_det(const float *img, const int64_t *img_strides, const float *flow,
                                           const float *grad_out, float *grad_img, float *grad_flow,
                                           int B, int C, int Hi, int Wi, int H, int W,
                                           int kernel_size, int bilinear, void *workspace, size_t workspace_bytes, void *stream)
{
    (void)bilinear;   // both reference backward kernels ignore the flag
    if (resample_dims_bad(B, C, Hi, Wi, H, W, kernel_size)) return FN2_EINVAL;
    if ((long)B * H * W == 0) return FN2_OK;
    if (any_null(img, flow, grad_out, grad_img, grad_flow)) return FN2_EINVAL;
    const size_t need = det_workspace_bytes((long)B * C, (long)Hi * Wi);
    if (!workspace || workspace_bytes < need) return FN2_EINVAL;
    if (!all_aligned(4, img, flow, grad_out, grad_img, grad_flow) || !aligned(workspace, 8)) return FN2_EALIGN;
    const ImgStrides is = dense_or(img_strides, C, Hi, Wi);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long npix = (long)B * H * W;
    DetSrc d{};
    d.gout = grad_out; d.C = C; d.HW = (long)H * W;
    DetAcc det{};
    int rc = det_begin<0>(d, B, workspace, need, det, det_K(kernel_size, H, W), s);
    if (rc != FN2_OK) return rc;
    // the atomic path's kernels with the scatter turned into fixed-point adds (same gather, same grad_flow); the tiled shapes take the
    // per-channel LDS-window kernel for every C, its window cells int64 instead of fp64
    if (kernel_size != 1) {
        hipLaunchKernelGGL(resample_bwd_ks_kernel<true>, dim3(stream_grid(npix)), dim3(256), 0, s, img, is, flow, grad_out, grad_img,
                           grad_flow, C, Hi, Wi, H, W, npix, kernel_size, det);
    } else if (tiled_shape_ok(is, img, Hi, Wi, H, W)) {
        const int tiles_x = (W + 63) / 64, tiles_y = (H + 31) / 32;
        hipLaunchKernelGGL((resample_bwd_tiled<32, 64, 16, 1024, 8, 2>), tile_grid(B, tiles_x, tiles_y), dim3(1024), 0, s, img, is, flow,
                           grad_out, grad_img, grad_flow, C, Hi, Wi, H, W, tiles_x, tiles_y, 0, det);
    } else {
        hipLaunchKernelGGL(resample_bwd_kernel<true>, dim3(stream_grid(npix)), dim3(256), 0, s, img, is, flow, grad_out, grad_img,
                           grad_flow, C, Hi, Wi, H, W, npix, det);
    }
    det_end<0>(d, flow, det, grad_img, (long)C * Hi * Wi, B, Hi, Wi, H, W, kernel_size, s);
    return launch_status();
}

extern "C" size_t fn2_warp_diff_norm_cat_backward_det_workspace_bytes(int B, int C, int H, int W)
{
    if (pair_dims_bad(B, C, H, W)) return 0;
    return det_workspace_bytes((long)B * C, (long)H * W);
}

extern "C" int fn2_warp_diff_norm_cat_backward_det(const float *pair, const float *flow, const float *out_cat, const float *grad_cat,
                                                   float *grad_pair, float *grad_flow, float div_flow, int B, int C, int H, int W,
                                                   int bilinear, void *workspace, size_t workspace_bytes, void *stream)
{
    if (pair_dims_bad(B, C, H, W, div_flow)) return FN2_EINVAL;
    if ((long)B * H * W == 0) return FN2_OK;
    if (any_null(pair, flow, out_cat, grad_cat, grad_flow)) return FN2_EINVAL;
    const size_t need = det_workspace_bytes((long)B * C, (long)H * W);
    if (!workspace || workspace_bytes < need) return FN2_EINVAL;
    if (!aligned(workspace, 8)) return FN2_EALIGN;
    // no pair gradient: nothing is scattered, the existing entry point is already deterministic
    if (!grad_pair) return fn2_warp_diff_norm_cat_backward(pair, flow, out_cat, grad_cat, nullptr, grad_flow, div_flow, B, C, H, W, bilinear, stream);
    if (!all_aligned(4, pair, flow, out_cat, grad_cat, grad_flow, grad_pair)) return FN2_EALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long HW = (long)H * W, npix = (long)B * HW;
    hipError_t e = seed_second_grad(grad_pair, grad_cat, B, C, HW, s);   // as on the atomic path
    if (e != hipSuccess) return (int)e;
    DetSrc d{};
    d.gcat = grad_cat; d.pair = pair; d.outcat = out_cat; d.C = C; d.HW = HW;
    DetAcc det{};
    int rc = det_begin<1>(d, B, workspace, need, det, det_K(1, H, W), s);
    if (rc != FN2_OK) return rc;
    // one lane per pixel for every shape: the first image's gradient, the gather of grad_flow and the fixed-point scatter (the arithmetic of
    // the tiled kernel, resample_bwd_c3x<..., 1, true>: same bits for grad_flow and grad_pair[:, :C])
    hipLaunchKernelGGL(warp_diff_norm_cat_bwd_kernel<true>, dim3(stream_grid(npix)), dim3(256), 0, s, pair, flow, out_cat, grad_cat, grad_pair,
                       grad_flow, C, H, W, npix, 1.0f / div_flow, 0, 1, det);
    det_end<1>(d, flow, det, grad_pair + (long)C * HW, 2L * C * HW, B, H, W, H, W, 1, s);
    return launch_status();
}
