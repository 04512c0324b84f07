// corr_sample1d.hip -- CorrSample1d: the lookup of a prebuilt 1-D correlation pyramid, RAFT-Stereo's CorrBlock1D
// (include/staging/flownet2_hip_sample1d.h), gfx950, float32.
//
//   out[b, l D + i, y, x] = w0 V(i) + w1 V(i+1)
//
// V(u), 0 <= u < G = 2 r + 2, is cell x0 - r + u of the query pixel's OWN slice of level l, x0 = floor(coords_x 2^-l).  No two
// query pixels share memory of a level: the forward is a gather of one G-cell window per (pixel, level), the backward writes
// every slice of every gradient level exactly once -- the grid weights wg(u) inside the window, +0 everywhere else -- without
// atomics or a clear.  One launch covers all levels; pointers and sizes come by value.
//
// This is not the 2-D kernel with a dimension dropped.  A window is G cells (40 bytes at r = 4) and the windows of consecutive
// pixels lie W2 cells apart, so the traffic is one short segment per (pixel, level) on the way in and, on the way back, slices
// as short as one or two cells at the coarse levels:
//
//   forward   a workgroup of 256 lanes owns NP = 32 consecutive pixels of one batch item.  It stages their windows of ALL levels
//             in LDS in one pass, 64 lanes to 64 / G windows -- consecutive lanes read consecutive cells of one window, and
//             NP G is a multiple of 64, so a wave works on one level and the level's pointer and width are scalars --, with the
//             odd pitch G + 1; a cell outside the level, or of a pixel without taps, is staged as +0 (the header: adding
//             w * (+0) gives the bits of leaving the term out).  One barrier.  Then lane (pixel, channel) mixes two cells per
//             output: a wave stores runs of NP consecutive pixels of one channel.
//   backward  a workgroup owns NP = 32 consecutive pixels: their grid weights of all levels go into LDS (grad_out read with the
//             pixels fastest, as it is stored), one barrier, then per level the lanes sweep the ONE contiguous span the pixels own
//             flat, four consecutive cells per lane, whichever slices they fall into -- 4-byte stores up to the first 16-byte
//             boundary, 16-byte stores, 4-byte stores for the rest.  Nothing is read back.
#include "corr_sample1d.h"

namespace fn2 {
namespace {

constexpr int NT = 256;
constexpr int ABSENT = -(1 << 30);   // x0 of a pixel without taps: every grid point lies left of the level, far from overflow

typedef float f4 __attribute__((ext_vector_type(4)));

// A finished output element or vector, written once: a plain C++ store.  (This library has no inline assembly, so it does not use
// fn2_common.h's store_out; measured against that form and against nontemporal stores in DESIGN.md 4.21.)
template <class V> __device__ __forceinline__ void put(V *p, V v) { *p = v; }

__device__ __forceinline__ bool inside(int v, int n) { return (unsigned)v < (unsigned)n; }
__device__ __forceinline__ float level_scale(int l) { return __uint_as_float((unsigned)(127 - l) << 23); }   // 2^-l
__device__ __forceinline__ bool has_taps(float c) { return fabsf(c) < 0x1p20f; }   // NaN compares false; before any float -> int

// which pixels a workgroup owns: NP consecutive ones of batch item b, from pix0 (row-major in H x W)
template <int NP> __device__ __forceinline__ void block_pixels(const Sample1dP &P, unsigned &HW, unsigned &b, unsigned &pix0)
{
    HW = (unsigned)P.H * (unsigned)P.W;
    const unsigned nblk = (HW + NP - 1) / NP;
    b = blockIdx.x / nblk;
    pix0 = (blockIdx.x % nblk) * NP;
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int R, int NP>
__global__ __launch_bounds__(NT) void sample1d_fwd(const float *__restrict__ cx, float *__restrict__ out, const Sample1dP P)
{
    constexpr int D = 2 * R + 1, G = D + 1, PITCH = G + 1, NK = NT / NP, PER_LEVEL = NP * G;
    static_assert(NT % NP == 0, "a wave stores whole runs of pixels");
    static_assert(PER_LEVEL % FN2_WAVE == 0, "the 64 cells a wave stages belong to one level");
    __shared__ float win[FN2H_MAX_LEVELS * NP * PITCH];   // win[(l NP + p) PITCH + u]
    const int tid = threadIdx.x;
    unsigned HW, b, pix0;
    block_pixels<NP>(P, HW, b, pix0);
    const float *cb = cx + (size_t)b * (size_t)P.cbs;
    const size_t slice0 = (size_t)b * HW + pix0;   // the first pixel's slice index

    const int total = P.L * PER_LEVEL;
    for (int e = tid; e < total; e += NT) {
        const int l = __builtin_amdgcn_readfirstlane(e / PER_LEVEL);   // wave-uniform (static_assert above)
        const int rem = e - l * PER_LEVEL, sp = rem / G, u = rem % G;  // u fastest: a pixel's window is contiguous
        const unsigned pix = pix0 + sp;
        float val = 0.f;
        if (pix < HW) {
            const float c = cb[pix];
            if (has_taps(c)) {
                const int W2 = P.W2[l], gx = (int)floorf(c * level_scale(l)) - R + u;
                if (inside(gx, W2)) val = P.lvl[l][(slice0 + sp) * (size_t)W2 + (size_t)gx];
            }
        }
        win[(l * NP + sp) * PITCH + u] = val;
    }
    __syncthreads();

    // this lane's own pixel in the mix
    const int p = tid % NP;
    const unsigned pix = pix0 + p;
    const bool inimg = pix < HW;
    float c = inimg ? cb[pix] : 0.f;
    if (!has_taps(c)) c = 0.f;   // (its windows are all +0)
    const int nch = P.L * D;
    float *op = out + (size_t)b * nch * HW + pix;
    for (int k = tid / NP; k < nch; k += NK) {
        const int l = k / D, i = k - l * D;
        const float sc = c * level_scale(l), fx = sc - floorf(sc), w0 = 1.f - fx;
        const float *pt = win + (l * NP + p) * PITCH + i;
        float s = 0.f;
        s = s + w0 * pt[0];
        s = s + fx * pt[1];
        if (inimg) put(op + (size_t)k * HW, s);
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
template <int R, int NP>
__global__ __launch_bounds__(NT) void sample1d_bwd(const float *__restrict__ cx, const float *__restrict__ go, const Sample1dP P)
{
    constexpr int D = 2 * R + 1, G = D + 1, PITCH = G + 1;
    __shared__ float wg[FN2H_MAX_LEVELS * NP * PITCH];   // wg[(l NP + p) PITCH + u]
    __shared__ unsigned sbx[FN2H_MAX_LEVELS * NP];       // x0 - r: the cell of grid point 0 (wrapped where negative)
    const int tid = threadIdx.x;
    unsigned HW, b, pix0;
    block_pixels<NP>(P, HW, b, pix0);
    const float *cb = cx + (size_t)b * (size_t)P.cbs;
    const unsigned np = min((unsigned)NP, HW - pix0);   // pixels of this workgroup inside the image
    const size_t slice0 = (size_t)b * HW + pix0;
    const int nch = P.L * D;

    // grid weights of every level: terms in the order (i, weight) = (u, w0) (u-1, w1), those whose tap exists
    const float *gob = go + (size_t)b * nch * HW;
    const int total = P.L * G * NP;
    for (int e = tid; e < total; e += NT) {
        const int p = e % NP, t = e / NP, l = t / G, u = t - l * G;   // pixels fastest: a channel's gO values are contiguous
        const unsigned pix = pix0 + p;
        float s = 0.f;
        int x0 = ABSENT;
        if (pix < HW) {
            const float c = cb[pix];
            if (has_taps(c)) {
                const float sc = c * level_scale(l), fl = floorf(sc), fx = sc - fl, w0 = 1.f - fx;
                x0 = (int)fl;
                const float *gop = gob + (size_t)(l * D) * HW + pix;
                if (u < D) s = s + gop[(size_t)u * HW] * w0;
                if (u >= 1) s = s + gop[(size_t)(u - 1) * HW] * fx;
            }
        }
        wg[(l * NP + p) * PITCH + u] = s;
        if (u == 0) sbx[l * NP + p] = (unsigned)(x0 - R);
    }
    __syncthreads();

    for (int l = 0; l < P.L; ++l) {
        const unsigned W2 = (unsigned)P.W2[l];
        float *dst = P.lvl[l] + slice0 * (size_t)W2;
        const float *wl = wg + l * NP * PITCH;
        const unsigned *bl = sbx + l * NP;
        // cell x of the q-th pixel's slice: wg inside the window [bx, bx + G), +0 outside (the difference wraps as intended)
        auto cell = [&](unsigned q, unsigned x) {
            const unsigned u = x - bl[q];
            return u < (unsigned)G ? wl[q * PITCH + u] : 0.f;
        };
        // the span of np W2 cells, flat; I is the index type: 32 bits unless the span needs more
        auto sweep = [&](auto span) {
            using I = decltype(span);
            const unsigned to16 = (4u - (unsigned)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u;
            const I head = (I)to16 < span ? (I)to16 : span, nv = (span - head) / 4, done = head + 4 * nv;
            for (I i = (I)tid; i < nv; i += NT) {
                const I c = head + 4 * i;
                unsigned q = (unsigned)(c / W2), x = (unsigned)(c - (I)q * W2);
                f4 val;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    val[k] = cell(q, x);
                    if (++x == W2) {
                        x = 0;
                        ++q;
                    }
                }
                put(reinterpret_cast<f4 *>(dst + c), val);
            }
            if ((I)tid < head) put(dst + tid, cell((unsigned)((I)tid / W2), (unsigned)((I)tid % W2)));
            if ((I)tid < span - done) {
                const I c = done + (I)tid;
                put(dst + c, cell((unsigned)(c / W2), (unsigned)(c % W2)));
            }
        };
        const size_t span = (size_t)np * W2;
        if (span <= 0xffffffffull) sweep((unsigned)span);
        else sweep(span);
    }
}

constexpr int NP_FWD = SAMPLE1D_TILE_FORWARD, NP_BWD = SAMPLE1D_TILE_BACKWARD;

unsigned blocks(const Sample1dP &p, int np) { return (unsigned)p.B * (unsigned)(((size_t)p.H * p.W + np - 1) / np); }

template <int R> int fwd_launch(const float *cx, float *out, const Sample1dP &p, hipStream_t s)
{
    hipLaunchKernelGGL((sample1d_fwd<R, NP_FWD>), dim3(blocks(p, NP_FWD)), dim3(NT), 0, s, cx, out, p);
    return launch_status();
}

template <int R> int bwd_launch(const float *cx, const float *go, const Sample1dP &p, hipStream_t s)
{
    hipLaunchKernelGGL((sample1d_bwd<R, NP_BWD>), dim3(blocks(p, NP_BWD)), dim3(NT), 0, s, cx, go, p);
    return launch_status();
}

} // namespace

#define FN2H_DISPATCH(fn, ...)                                                                                                         \
    switch (p.r) {                                                                                                                     \
    case 0: return fn<0>(__VA_ARGS__);                                                                                                 \
    case 1: return fn<1>(__VA_ARGS__);                                                                                                 \
    case 2: return fn<2>(__VA_ARGS__);                                                                                                 \
    case 3: return fn<3>(__VA_ARGS__);                                                                                                 \
    case 4: return fn<4>(__VA_ARGS__);                                                                                                 \
    case 5: return fn<5>(__VA_ARGS__);                                                                                                 \
    case 6: return fn<6>(__VA_ARGS__);                                                                                                 \
    case 7: return fn<7>(__VA_ARGS__);                                                                                                 \
    case 8: return fn<8>(__VA_ARGS__);                                                                                                 \
    }                                                                                                                                  \
    return FN2_EINVAL;

int sample1d_forward(const float *cx, float *out, const Sample1dP &p, hipStream_t s) { FN2H_DISPATCH(fwd_launch, cx, out, p, s) }

int sample1d_backward(const float *cx, const float *go, const Sample1dP &p, hipStream_t s) { FN2H_DISPATCH(bwd_launch, cx, go, p, s) }

} // namespace fn2
