// resample2d_lowp.hip -- the fused warp rows (fn2_warp_diff_norm_cat, fn2_warp_diff_norm and their flow-gradient backward passes) on half
// and bfloat16 tensors for gfx950: 16 bits in memory, the float32 kernels' arithmetic inside.
//
// Contract (include/flownet2_hip.h): every element written has the bits of the float32 entry point run on the exactly widened inputs,
// its float32 result rounded to the 16-bit type once (round to nearest even; overflow -> inf, subnormal results kept, NaN stays NaN).
// So the expressions below are those of resample2d.hip in the same order (shared helpers: resample2d_common.h; the library is built
// without contraction), the norm is taken from the UNROUNDED warped values, and the backward kernels never read a warped value or a
// norm from a 16-bit tensor: they recompute both from the pair and the flow with the forward's arithmetic.
//
// Tiled kernels (C == 3, H >= 16, W >= 32, W % 8 == 0, 16-byte aligned tensors): a 256-thread workgroup owns a 32 x 64 tile, each lane
// EIGHT adjacent pixels of one row: every input plane arrives as one 16-byte load per lane, every output plane leaves as one 16-byte
// store (the vector-memory path retires instructions, not bytes; 2-byte stores cost an order of magnitude more per byte, DESIGN.md
// 4.2c).  The three channels of the second image's window (tile +- 16 px) sit in LDS in 16 bits -- widening is exact, and the
// window is half the float32 kernels': 64 x 96 x 3 x 2 B = 36 KB, four workgroups (16 waves) per CU, one barrier per kernel.  Corners
// outside the window are read from global memory as the aligned 32-bit word that holds them.
// Everything else (C != 3, small or ragged maps, planes that are only 2-byte aligned): one lane per pixel, same arithmetic.
#include "fn2_common.h"
#include "resample2d_common.h"

namespace fn2 {

typedef unsigned __attribute__((ext_vector_type(4))) u4;
typedef unsigned short us;

// widening (exact) and the single rounding of a result (Op16<T>::pk: v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32, round to nearest even)
template <class T> struct Lowp;
template <> struct Lowp<half_t> {
    static __device__ __forceinline__ float widen(unsigned bits) { return (float)__builtin_bit_cast(half_t, (us)bits); }
};
template <> struct Lowp<bf16_t> {
    static __device__ __forceinline__ float widen(unsigned bits) { return __uint_as_float(bits << 16); }
};
template <class T> __device__ __forceinline__ us narrow(float v)
{
    // the float32 value is final: keep the compiler from folding the operation that made it into the conversion (v_fma_mixlo_f16
    // rounds the exact product or sum to half ONCE, where the contract rounds to float32 first)
    asm volatile("" : "+v"(v));
    return (us)(Op16<T>::pk(v, 0.0f) & 0xffffu);
}
template <class T> __device__ __forceinline__ u4 narrow8(const float v[8])
{
    return (u4){Op16<T>::pk(v[0], v[1]), Op16<T>::pk(v[2], v[3]), Op16<T>::pk(v[4], v[5]), Op16<T>::pk(v[6], v[7])};
}
__device__ __forceinline__ unsigned elem16(const u4 &v, int k) { return (v[k >> 1] >> ((k & 1) * 16)) & 0xffffu; }
// word j of a vector for a j only known at run time, by selects (an indexed register access would go through scratch)
__device__ __forceinline__ unsigned sel4(const u4 &v, int j) { return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3])); }
__device__ __forceinline__ void put4(u4 &v, int j, unsigned w)
{
    v[0] = j == 0 ? w : v[0]; v[1] = j == 1 ? w : v[1]; v[2] = j == 2 ? w : v[2]; v[3] = j == 3 ? w : v[3];
}

// The norm's square root is sqrtf, correctly rounded, as in the float32 kernels (channelnorm.hip, resample2d.hip): every path has the bits
// of the float32 entry point on the widened inputs, whichever kernel that entry point takes for the shape.
// MODE 0: fn2_warp_diff_norm_cat_16   1: fn2_warp_diff_norm_16   2: fn2_warp_diff_norm_cat_backward_16   3: fn2_warp_diff_norm_backward_16
struct Warp16Args {
    const us *pair, *flow;
    const us *grad;            // MODE 2: B x (3C+3) x H x W concat gradient; MODE 3: B x 1 x H x W gradient of the norm
    us *out;                   // MODE 0: B x (3C+3) x H x W; MODE 1: B x 1 x H x W; MODE 2, 3: B x 2 x H x W flow gradient
    int B, C, H, W, tiles_x, tiles_y, bilinear;
    float inv_div_flow;
};

template <class T, int MODE>
__global__ __launch_bounds__(256) void warp16_tiled(const Warp16Args p)
{
    constexpr int TH = 32, TW = 64, R = 16, NT = 256, WH = TH + 2 * R, WW = TW + 2 * R, GPR = WW / 8, NG = WH * GPR, NW = NG / NT, C = 3;
    constexpr bool BWD = MODE >= 2;
    static_assert(NG % NT == 0, "whole 8-pixel groups per thread");
    __shared__ __attribute__((aligned(16))) us win[C][WH * WW];

    const int tid = threadIdx.x;
    int t = (int)xcd_remap(blockIdx.x, gridDim.x);   // an XCD's workgroups take consecutive tiles: neighbours share its L2
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y;
    const int b = t / p.tiles_y;
    const int H = p.H, W = p.W, bilinear = p.bilinear;
    const int X0 = tx * TW, Y0 = ty * TH, wx0 = X0 - R, wy0 = Y0 - R;
    const long HW = (long)H * W;
    const us *const img = p.pair + ((long)b * 2 * C + C) * HW;   // the image that is warped

    // the window: 8-pixel groups, entirely inside or outside the image (W % 8 == 0, wx0 % 8 == 0); outside is never gathered (corners
    // are clamped to the image)
    u4 wreg[C][NW];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int i = tid + NT * j;
            const int ly = i / GPR, lx = (i - ly * GPR) * 8;
            const int gy = wy0 + ly, gx = wx0 + lx;
            u4 v = (u4){0u, 0u, 0u, 0u};
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const u4 *>(img + (long)c * HW + (long)gy * W + gx);
            wreg[c][j] = v;
        }
    // the lane's eight pixels
    const int x0 = X0 + 8 * (tid & 7), y = Y0 + (tid >> 3);
    const bool live = x0 < W && y < H;
    const long pix0 = live ? (long)y * W + x0 : 0;
    const u4 fdx = *reinterpret_cast<const u4 *>(p.flow + (long)b * 2 * HW + pix0);
    const u4 fdy = *reinterpret_cast<const u4 *>(p.flow + (long)b * 2 * HW + HW + pix0);
    u4 first[C];
#pragma unroll
    for (int c = 0; c < C; ++c) first[c] = *reinterpret_cast<const u4 *>(p.pair + ((long)b * 2 * C + c) * HW + pix0);
    u4 gw[MODE == 2 ? C : 1], gf[MODE == 2 ? 2 : 1], gn = (u4){0u, 0u, 0u, 0u};
    if constexpr (MODE == 2) {
        const us *gb = p.grad + (long)b * (3 * C + 3) * HW + pix0;
#pragma unroll
        for (int c = 0; c < C; ++c) gw[c] = *reinterpret_cast<const u4 *>(gb + (long)(2 * C + c) * HW);
        gf[0] = *reinterpret_cast<const u4 *>(gb + (long)(3 * C) * HW);
        gf[1] = *reinterpret_cast<const u4 *>(gb + (long)(3 * C + 1) * HW);
        gn = *reinterpret_cast<const u4 *>(gb + (long)(3 * C + 2) * HW);
    } else if constexpr (MODE == 3) {
        gn = *reinterpret_cast<const u4 *>(p.grad + (long)b * HW + pix0);
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < NW; ++j) *reinterpret_cast<u4 *>(&win[c][8 * (tid + NT * j)]) = wreg[c][j];
    __syncthreads();
    if (!live) return;

    // one pixel: its 16-bit inputs in, the forward's values (val, nrm) or the flow gradient (odx, ody) out
    auto pixel = [&](int x, unsigned bdx, unsigned bdy, const unsigned bfirst[C], unsigned bgn, const unsigned bgw[C], unsigned bgfx,
                     unsigned bgfy, float val[C], float &nrm, float &odx, float &ody) __attribute__((always_inline)) {
        const WarpPos q = warp_pos<BWD>(x, y, Lowp<T>::widen(bdx), Lowp<T>::widen(bdy), H, W, bilinear);
        const int lxL = q.xL - wx0, lxR = q.xR - wx0, lyT = q.yT - wy0, lyB = q.yB - wy0;
        const bool in = (lxL >= 0) && (lxR < WW) && (lyT >= 0) && (lyB < WH);
        float cr[C][4];
        if (in) {
            const int o = lyT * WW + lxL, ox = lxR - lxL, oy = (lyB - lyT) * WW;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                cr[c][0] = Lowp<T>::widen(win[c][o]); cr[c][1] = Lowp<T>::widen(win[c][o + ox]);
                cr[c][2] = Lowp<T>::widen(win[c][o + oy]); cr[c][3] = Lowp<T>::widen(win[c][o + oy + ox]);
            }
        } else {   // far sample: the aligned 32-bit word that holds the corner (planes are 16-byte aligned and even-sized)
            const int e[4] = {q.yT * W + q.xL, q.yT * W + q.xR, q.yB * W + q.xL, q.yB * W + q.xR};
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const unsigned w32 = *reinterpret_cast<const unsigned *>(img + (long)c * HW + (e[n] & ~1));
                    cr[c][n] = Lowp<T>::widen((w32 >> ((e[n] & 1) * 16)) & 0xffffu);
                }
        }
        float diff[C], ssq = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            val[c] = warp_value<BWD>(q, bilinear, cr[c][0], cr[c][1], cr[c][2], cr[c][3]);
            diff[c] = Lowp<T>::widen(bfirst[c]) - val[c];   // models.py:134
            ssq = ssq + diff[c] * diff[c];                  // channelnorm_kernel.cu:47-50
        }
        nrm = sqrtf(ssq);                                   // channelnorm_kernel.cu:52
        if constexpr (BWD) {
            const float gnk = Lowp<T>::widen(bgn);
            const float gam_y = 1 - q.alpha, gam_x = 1 - q.beta;      // (:169, :182)
            float out_dx = 0.0f, out_dy = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float gd = chnorm_grad(gnk, diff[c], nrm);
                const float g = MODE == 2 ? Lowp<T>::widen(bgw[c]) - gd : 0.0f - gd;
                flow_grad_terms(out_dx, out_dy, gam_x, gam_y, g, cr[c][0], cr[c][1], cr[c][2], cr[c][3]);
            }
            if constexpr (MODE == 2) {   // + the gradient through flow / div_flow = flow * (1 / div_flow) (models.py:137)
                out_dx = out_dx + Lowp<T>::widen(bgfx) * p.inv_div_flow;
                out_dy = out_dy + Lowp<T>::widen(bgfy) * p.inv_div_flow;
            }
            odx = out_dx; ody = out_dy;
        }
    };
    if constexpr (BWD) {
        // two pixels (one 32-bit word of every plane) per trip of a loop that is NOT unrolled: unrolled, the eight pixels' gathers are
        // hoisted together and the kernel needs ~190 registers (2 waves per SIMD)
        u4 ox4 = (u4){0u, 0u, 0u, 0u}, oy4 = ox4;
#pragma unroll 1
        for (int kk = 0; kk < 4; ++kk) {
            const unsigned wdx = sel4(fdx, kk), wdy = sel4(fdy, kk), wgn = sel4(gn, kk);
            const unsigned wf[C] = {sel4(first[0], kk), sel4(first[1], kk), sel4(first[2], kk)};
            unsigned wg[C] = {0u, 0u, 0u}, wfx = 0u, wfy = 0u;
            if constexpr (MODE == 2) {
                wg[0] = sel4(gw[0], kk); wg[1] = sel4(gw[1], kk); wg[2] = sel4(gw[2], kk);
                wfx = sel4(gf[0], kk); wfy = sel4(gf[1], kk);
            }
            float odx[2], ody[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int sh = 16 * h;
                const unsigned bf[C] = {(wf[0] >> sh) & 0xffffu, (wf[1] >> sh) & 0xffffu, (wf[2] >> sh) & 0xffffu};
                const unsigned bg[C] = {(wg[0] >> sh) & 0xffffu, (wg[1] >> sh) & 0xffffu, (wg[2] >> sh) & 0xffffu};
                float val[C], nrm;
                pixel(x0 + 2 * kk + h, (wdx >> sh) & 0xffffu, (wdy >> sh) & 0xffffu, bf, (wgn >> sh) & 0xffffu, bg, (wfx >> sh) & 0xffffu,
                      (wfy >> sh) & 0xffffu, val, nrm, odx[h], ody[h]);
            }
            put4(ox4, kk, Op16<T>::pk(odx[0], odx[1]));
            put4(oy4, kk, Op16<T>::pk(ody[0], ody[1]));
        }
        store_out(reinterpret_cast<u4 *>(p.out + (long)b * 2 * HW + pix0), ox4);
        store_out(reinterpret_cast<u4 *>(p.out + (long)b * 2 * HW + HW + pix0), oy4);
        return;
    }
    float r0[8], r1[8], r2[8], rn[8];   // the warped channels and the norm
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned bf[C] = {elem16(first[0], k), elem16(first[1], k), elem16(first[2], k)};
        const unsigned none[C] = {0u, 0u, 0u};
        float val[C], odx, ody;
        pixel(x0 + k, elem16(fdx, k), elem16(fdy, k), bf, 0u, none, 0u, 0u, val, rn[k], odx, ody);
        r0[k] = val[0]; r1[k] = val[1]; r2[k] = val[2];
    }
    if constexpr (MODE == 0) {
        us *ob = p.out + (long)b * (3 * C + 3) * HW + pix0;
        const int self = ((tid >> 3) + R) * WW + R + 8 * (tid & 7);   // the lane's own pixels are always inside the window
#pragma unroll
        for (int c = 0; c < C; ++c) {
            store_out(reinterpret_cast<u4 *>(ob + (long)c * HW), first[c]);
            store_out(reinterpret_cast<u4 *>(ob + (long)(C + c) * HW), *reinterpret_cast<const u4 *>(&win[c][self]));
        }
        store_out(reinterpret_cast<u4 *>(ob + (long)(2 * C) * HW), narrow8<T>(r0));
        store_out(reinterpret_cast<u4 *>(ob + (long)(2 * C + 1) * HW), narrow8<T>(r1));
        store_out(reinterpret_cast<u4 *>(ob + (long)(2 * C + 2) * HW), narrow8<T>(r2));
        float fx8[8], fy8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            fx8[k] = Lowp<T>::widen(elem16(fdx, k)) * p.inv_div_flow;
            fy8[k] = Lowp<T>::widen(elem16(fdy, k)) * p.inv_div_flow;
        }
        store_out(reinterpret_cast<u4 *>(ob + (long)(3 * C) * HW), narrow8<T>(fx8));
        store_out(reinterpret_cast<u4 *>(ob + (long)(3 * C + 1) * HW), narrow8<T>(fy8));
        store_out(reinterpret_cast<u4 *>(ob + (long)(3 * C + 2) * HW), narrow8<T>(rn));
    } else if constexpr (MODE == 1) {
        store_out(reinterpret_cast<u4 *>(p.out + (long)b * HW + pix0), narrow8<T>(rn));
    }
}

// Every shape the tiled kernels decline: one lane per pixel, corners gathered from global memory, 2-byte accesses.
template <class T, int MODE>
__global__ __launch_bounds__(256) void warp16_pixel(const Warp16Args p, long npix)
{
    constexpr bool BWD = MODE >= 2;
    const int C = p.C, H = p.H, W = p.W, bilinear = p.bilinear;
    const long HW = (long)H * W;
    const int CC = 3 * C + 3;
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < npix; g += (long)gridDim.x * blockDim.x) {
        const int x = (int)(g % W);
        const long row = g / W;
        const int y = (int)(row % H), b = (int)(row / H);
        const long pix = (long)y * W + x;
        const float dx = Lowp<T>::widen(p.flow[(long)b * 2 * HW + pix]), dy = Lowp<T>::widen(p.flow[(long)b * 2 * HW + HW + pix]);
        const WarpPos q = warp_pos<BWD>(x, y, dx, dy, H, W, bilinear);
        const long eTL = (long)q.yT * W + q.xL, eTR = (long)q.yT * W + q.xR, eBL = (long)q.yB * W + q.xL, eBR = (long)q.yB * W + q.xR;
        const us *first = p.pair + (long)b * 2 * C * HW + pix, *img = p.pair + ((long)b * 2 * C + C) * HW;
        float ssq = 0.0f;
        for (int c = 0; c < C; ++c) {
            const us *I = img + (long)c * HW;
            const float val = warp_value<BWD>(q, bilinear, Lowp<T>::widen(I[eTL]), Lowp<T>::widen(I[eTR]), Lowp<T>::widen(I[eBL]),
                                              Lowp<T>::widen(I[eBR]));
            const float d = Lowp<T>::widen(first[(long)c * HW]) - val;
            ssq = ssq + d * d;
            if constexpr (MODE == 0) {
                us *ob = p.out + (long)b * CC * HW + pix;
                ob[(long)c * HW] = first[(long)c * HW];
                ob[(long)(C + c) * HW] = I[pix];
                ob[(long)(2 * C + c) * HW] = narrow<T>(val);
            }
        }
        const float nrm = sqrtf(ssq);
        if constexpr (MODE == 0) {
            us *ob = p.out + (long)b * CC * HW + pix;
            ob[(long)(3 * C) * HW] = narrow<T>(dx * p.inv_div_flow);
            ob[(long)(3 * C + 1) * HW] = narrow<T>(dy * p.inv_div_flow);
            ob[(long)(3 * C + 2) * HW] = narrow<T>(nrm);
        } else if constexpr (MODE == 1) {
            p.out[(long)b * HW + pix] = narrow<T>(nrm);
        } else {
            const us *gb = MODE == 2 ? p.grad + (long)b * CC * HW + pix : p.grad + (long)b * HW + pix;
            const float gn = Lowp<T>::widen(MODE == 2 ? gb[(long)(3 * C + 2) * HW] : gb[0]);
            const float gam_y = 1 - q.alpha, gam_x = 1 - q.beta;
            float out_dx = 0.0f, out_dy = 0.0f;
            for (int c = 0; c < C; ++c) {   // the warp once more, now that the norm is known
                const us *I = img + (long)c * HW;
                const float iTL = Lowp<T>::widen(I[eTL]), iTR = Lowp<T>::widen(I[eTR]), iBL = Lowp<T>::widen(I[eBL]), iBR = Lowp<T>::widen(I[eBR]);
                const float val = warp_value<BWD>(q, bilinear, iTL, iTR, iBL, iBR);
                const float gd = chnorm_grad(gn, Lowp<T>::widen(first[(long)c * HW]) - val, nrm);
                float go = 0.0f - gd;
                if constexpr (MODE == 2) go = Lowp<T>::widen(gb[(long)(2 * C + c) * HW]) - gd;
                flow_grad_terms(out_dx, out_dy, gam_x, gam_y, go, iTL, iTR, iBL, iBR);
            }
            if constexpr (MODE == 2) {
                out_dx = out_dx + Lowp<T>::widen(gb[(long)(3 * C) * HW]) * p.inv_div_flow;
                out_dy = out_dy + Lowp<T>::widen(gb[(long)(3 * C + 1) * HW]) * p.inv_div_flow;
            }
            p.out[(long)b * 2 * HW + pix] = narrow<T>(out_dx);
            p.out[(long)b * 2 * HW + HW + pix] = narrow<T>(out_dy);
        }
    }
}

} // namespace fn2

template <class T, int MODE> static int warp16_launch(const fn2::Warp16Args &a, bool tiled, hipStream_t s)
{
    using namespace fn2;
    if (tiled) {
        hipLaunchKernelGGL((warp16_tiled<T, MODE>), dim3((unsigned)((long)a.B * a.tiles_x * a.tiles_y)), dim3(256), 0, s, a);
    } else {
        const long npix = (long)a.B * a.H * a.W;
        hipLaunchKernelGGL((warp16_pixel<T, MODE>), dim3(stream_grid(npix)), dim3(256), 0, s, a, npix);
    }
    return launch_status();
}

// Checks in the order of the float32 entry points (element type first), then the launch.  `grad`: null for the forward modes.
template <int MODE>
static int warp16(const void *pair, const void *flow, const void *grad, void *out, int dtype, float div_flow, int B, int C, int H, int W,
                  int bilinear, void *stream)
{
    using namespace fn2;
    if (dtype != FN2_F16 && dtype != FN2_BF16) return FN2_EDTYPE;
    if (B < 0 || C < 1 || H < 1 || W < 1 || !(div_flow == div_flow) || div_flow == 0.0f) return FN2_EINVAL;
    if ((long)B * H * W == 0) return FN2_OK;
    if (!pair || !flow || !out || (MODE >= 2 && !grad)) return FN2_EINVAL;
    if (!aligned(pair, 2) || !aligned(flow, 2) || !aligned(out, 2) || (MODE >= 2 && !aligned(grad, 2))) return FN2_EALIGN;
    Warp16Args a;
    a.pair = static_cast<const us *>(pair); a.flow = static_cast<const us *>(flow); a.grad = static_cast<const us *>(grad);
    a.out = static_cast<us *>(out);
    a.B = B; a.C = C; a.H = H; a.W = W; a.tiles_x = (W + 63) / 64; a.tiles_y = (H + 31) / 32; a.bilinear = bilinear != 0 ? 1 : 0;
    a.inv_div_flow = 1.0f / div_flow;   // as PyTorch divides a GPU tensor by a scalar
    const bool tiled = C == 3 && H >= 16 && W >= 32 && W % 8 == 0 && aligned(pair, 16) && aligned(flow, 16) && aligned(out, 16) &&
                       (MODE < 2 || aligned(grad, 16));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == FN2_F16 ? warp16_launch<half_t, MODE>(a, tiled, s) : warp16_launch<bf16_t, MODE>(a, tiled, s);
}

extern "C" int fn2_warp_diff_norm_cat_16(const void *pair, const void *flow, void *out, int dtype, float div_flow, int B, int C, int H, int W,
                                         int bilinear, void *stream)
{
    return warp16<0>(pair, flow, nullptr, out, dtype, div_flow, B, C, H, W, bilinear, stream);
}

extern "C" int fn2_warp_diff_norm_16(const void *pair, const void *flow, void *out_norm, int dtype, int B, int C, int H, int W, int bilinear,
                                     void *stream)
{
    return warp16<1>(pair, flow, nullptr, out_norm, dtype, 1.0f, B, C, H, W, bilinear, stream);
}

extern "C" int fn2_warp_diff_norm_cat_backward_16(const void *pair, const void *flow, const void *grad_cat, void *grad_flow, int dtype,
                                                  float div_flow, int B, int C, int H, int W, int bilinear, void *stream)
{
    return warp16<2>(pair, flow, grad_cat, grad_flow, dtype, div_flow, B, C, H, W, bilinear, stream);
}

extern "C" int fn2_warp_diff_norm_backward_16(const void *pair, const void *flow, const void *grad_norm, void *grad_flow, int dtype, int B,
                                              int C, int H, int W, int bilinear, void *stream)
{
    return warp16<3>(pair, flow, grad_norm, grad_flow, dtype, 1.0f, B, C, H, W, bilinear, stream);
}
