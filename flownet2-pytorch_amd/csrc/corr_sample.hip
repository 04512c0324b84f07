// corr_sample.hip -- CorrSample: the lookup of a prebuilt all-pairs correlation pyramid, RAFT's CorrBlock
// (include/preview/flownet2_hip_sample.h), gfx950, float32.
//
//   out[b, l D^2 + i D + j, y, x] = ((w00 V(i,j) + w10 V(i+1,j)) + w01 V(i,j+1)) + w11 V(i+1,j+1)
//
// V(u,v), 0 <= u,v < G = 2 r + 2, is cell (x0 - r + u, y0 - r + v) of the query pixel's OWN slice of level l, (x0, y0) =
// floor(coords 2^-l).  No two query pixels share memory of a level: the forward is a gather of one G x G patch per (pixel,
// level), the backward writes every slice of every gradient level exactly once -- the grid weights wg(u,v) inside the patch's
// box, +0 everywhere else -- without atomics or a clear.  One launch covers all levels; pointers and sizes come by value.
//
//   forward   a workgroup of 256 lanes owns NP consecutive pixels of one batch item.  Per level it stages their patches in LDS,
//             pixel-major with the odd pitch G^2 + 1 (lanes that read one cell index of different pixels hit different banks);
//             a cell outside the level, or of a pixel without taps, is staged as +0 (the header: adding w * (+0) gives the bits
//             of leaving the term out).  Then lane (pixel, channel group) mixes four cells per output: a wave stores runs of NP
//             consecutive pixels of one channel.
//   backward  a workgroup owns NP consecutive pixels: their grid weights per level go into LDS, then the lanes sweep the
//             pixels' slices one after the other -- 4-byte stores up to the first 16-byte boundary, 16-byte stores, 4-byte
//             stores for the rest.  Nothing is read back.
#include "corr_sample.h"

namespace fn2 {
namespace {

constexpr int NT = 256;
constexpr int ABSENT = -(1 << 30);   // y0 of a pixel without taps: every grid row lies above the level, far from overflow

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool inside(int v, int n) { return (unsigned)v < (unsigned)n; }
__device__ __forceinline__ float level_scale(int l) { return __uint_as_float((unsigned)(127 - l) << 23); }   // 2^-l
// NaN compares false; before any float -> int conversion
__device__ __forceinline__ bool has_taps(float cx, float cy) { return (fabsf(cx) < 0x1p20f) && (fabsf(cy) < 0x1p20f); }

struct Weights {
    float w00, w10, w01, w11;
};

__device__ __forceinline__ Weights weights(float fx, float fy)
{
    const float ux = 1.f - fx, uy = 1.f - fy;
    return Weights{ux * uy, fx * uy, ux * fy, fx * fy};
}

// which pixels a workgroup owns: NP consecutive ones of batch item b, from pix0 (row-major in H x W)
template <int NP> __device__ __forceinline__ void block_pixels(const SampleP &P, unsigned &HW, unsigned &b, unsigned &pix0)
{
    HW = (unsigned)P.H * (unsigned)P.W;
    const unsigned nblk = (HW + NP - 1) / NP;
    b = blockIdx.x / nblk;
    pix0 = (blockIdx.x % nblk) * NP;
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int R, int NP>
__global__ __launch_bounds__(NT) void sample_fwd(const float *__restrict__ co, float *__restrict__ out, const SampleP P)
{
    constexpr int D = 2 * R + 1, G = D + 1, GG = G * G, PITCH = GG + 1, NK = NT / NP, ITER = (NP * GG + NT - 1) / NT;
    constexpr int UNROLL = ITER <= 16 ? ITER : 8;
    static_assert(NT % NP == 0, "a wave stores whole runs of pixels");
    __shared__ float patch[NP * PITCH];
    __shared__ int sx0[FN2P_MAX_LEVELS][NP], sy0[FN2P_MAX_LEVELS][NP];
    const int tid = threadIdx.x;
    unsigned HW, b, pix0;
    block_pixels<NP>(P, HW, b, pix0);
    const float *cob = co + (size_t)b * 2 * HW;

    // floor(coords 2^-l) of the workgroup's pixels, every level; a pixel without taps or beyond the image is ABSENT
    for (int e = tid; e < P.L * NP; e += NT) {
        const int l = e / NP, p = e % NP;
        const unsigned pix = pix0 + p;
        int x0 = 0, y0 = ABSENT;
        if (pix < HW) {
            const float cx = cob[pix], cy = cob[HW + pix];
            if (has_taps(cx, cy)) {
                x0 = (int)floorf(cx * level_scale(l));
                y0 = (int)floorf(cy * level_scale(l));
            }
        }
        sx0[l][p] = x0;
        sy0[l][p] = y0;
    }

    // this lane's own pixel in the mix
    const int p = tid % NP;
    const unsigned pix = pix0 + p;
    const bool inimg = pix < HW;
    float cx = 0.f, cy = 0.f;
    if (inimg) {
        cx = cob[pix];
        cy = cob[HW + pix];
    }
    if (!has_taps(cx, cy)) cx = cy = 0.f;   // (its patches are all +0)
    const size_t slice0 = (size_t)b * HW + pix0;   // the first pixel's slice index

    for (int l = 0; l < P.L; ++l) {
        __syncthreads();   // l == 0: sx0, sy0 are published; later: the previous level's patches have been read
        const int H2 = P.H2[l], W2 = P.W2[l];
        const size_t S = (size_t)H2 * W2;
        const float *lv = P.lvl[l];
#pragma unroll UNROLL   // the loads of UNROLL cells are in flight together
        for (int k = 0; k < ITER; ++k) {
            const int e = tid + k * NT;
            if (e < NP * GG) {
                const int sp = e / GG, c = e % GG, v = c / G, u = c % G;   // u fastest: a pixel's row segment is contiguous
                const int gx = sx0[l][sp] - R + u, gy = sy0[l][sp] - R + v;
                float val = 0.f;
                if (inside(gx, W2) && inside(gy, H2)) val = lv[(slice0 + sp) * S + (size_t)gy * W2 + gx];
                patch[sp * PITCH + c] = val;
            }
        }
        __syncthreads();
        const float sx = cx * level_scale(l), sy = cy * level_scale(l);
        const Weights w = weights(sx - floorf(sx), sy - floorf(sy));
        const float *pt = patch + p * PITCH;
        float *op = out + ((size_t)b * P.L + l) * (D * D) * HW + pix;
        for (int k = tid / NP; k < D * D; k += NK) {
            const int i = k / D, j = k % D, c = j * G + i;
            float s = 0.f;
            s = s + w.w00 * pt[c];
            s = s + w.w10 * pt[c + 1];
            s = s + w.w01 * pt[c + G];
            s = s + w.w11 * pt[c + G + 1];
            if (inimg) store_out(op + (size_t)k * HW, s);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
template <int R, int NP>
__global__ __launch_bounds__(NT) void sample_bwd(const float *__restrict__ co, const float *__restrict__ go, const SampleP P)
{
    constexpr int D = 2 * R + 1, G = D + 1, GG = G * G, PITCH = GG + 1;
    __shared__ float wg[NP * PITCH];   // wg[p PITCH + v G + u]
    __shared__ int sx0[NP], sy0[NP];
    __shared__ float sfx[NP], sfy[NP];
    const int tid = threadIdx.x;
    unsigned HW, b, pix0;
    block_pixels<NP>(P, HW, b, pix0);
    const float *cob = co + (size_t)b * 2 * HW;
    const unsigned np = min((unsigned)NP, HW - pix0);   // pixels of this workgroup inside the image
    const size_t slice0 = (size_t)b * HW + pix0;

    for (int l = 0; l < P.L; ++l) {
        __syncthreads();   // the previous level's sweep has read wg, sx0, sy0
        if (tid < NP) {
            const unsigned pix = pix0 + tid;
            int x0 = 0, y0 = ABSENT;
            float fx = 0.f, fy = 0.f;
            if (pix < HW) {
                const float cx = cob[pix], cy = cob[HW + pix];
                if (has_taps(cx, cy)) {
                    const float sx = cx * level_scale(l), sy = cy * level_scale(l);
                    const float flx = floorf(sx), fly = floorf(sy);
                    x0 = (int)flx;
                    y0 = (int)fly;
                    fx = sx - flx;
                    fy = sy - fly;
                }
            }
            sx0[tid] = x0;
            sy0[tid] = y0;
            sfx[tid] = fx;
            sfy[tid] = fy;
        }
        __syncthreads();
        // grid weights: terms in the order (i,j,corner) = (u,v,00) (u-1,v,10) (u,v-1,01) (u-1,v-1,11), those whose tap exists
        const float *gob = go + ((size_t)b * P.L + l) * (D * D) * HW + pix0;
        for (int e = tid; e < NP * GG; e += NT) {
            const int p = e % NP, g = e / NP, v = g / G, u = g % G;   // pixels fastest: a channel's gO values are contiguous
            float s = 0.f;
            if (sy0[p] != ABSENT) {
                const Weights w = weights(sfx[p], sfy[p]);
                const float *gop = gob + p;
                if (u < D && v < D) s = s + gop[(size_t)(u * D + v) * HW] * w.w00;
                if (u >= 1 && v < D) s = s + gop[(size_t)((u - 1) * D + v) * HW] * w.w10;
                if (u < D && v >= 1) s = s + gop[(size_t)(u * D + v - 1) * HW] * w.w01;
                if (u >= 1 && v >= 1) s = s + gop[(size_t)((u - 1) * D + v - 1) * HW] * w.w11;
            }
            wg[p * PITCH + g] = s;
        }
        __syncthreads();
        // the sweep: slice q of this level, cell c = y W2 + x, is wg inside the box [bx, bx + G) x [by, by + G) and +0 outside
        const unsigned H2 = P.H2[l], W2 = P.W2[l], S = H2 * W2;   // S < 2^31
        for (unsigned q = 0; q < np; ++q) {
            float *dst = P.lvl[l] + (slice0 + q) * (size_t)S;
            const float *wq = wg + q * PITCH;
            const unsigned bx = (unsigned)(sx0[q] - R), by = (unsigned)(sy0[q] - R);   // (differences below wrap as intended)
            auto cell = [&](unsigned x, unsigned y) {
                const unsigned u = x - bx, v = y - by;
                return (u < (unsigned)G && v < (unsigned)G) ? wq[v * G + u] : 0.f;
            };
            const unsigned to16 = (4u - (unsigned)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u;
            const unsigned head = min(to16, S), nv = (S - head) / 4, done = head + 4 * nv;
            for (unsigned i = tid; i < nv; i += NT) {
                const unsigned c = head + 4 * i;
                unsigned y = c / W2, x = c - y * W2;
                f4 val;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    val[k] = cell(x, y);
                    if (++x == W2) {
                        x = 0;
                        ++y;
                    }
                }
                store_out(reinterpret_cast<f4 *>(dst + c), val);
            }
            if ((unsigned)tid < head) store_out(dst + tid, cell(tid % W2, tid / W2));
            if ((unsigned)tid < S - done) store_out(dst + done + tid, cell((done + tid) % W2, (done + tid) / W2));
        }
    }
}

constexpr int NP_FWD = FN2P_TILE_FORWARD, NP_BWD = FN2P_TILE_BACKWARD;

unsigned blocks(const SampleP &p, int np) { return (unsigned)p.B * (unsigned)(((size_t)p.H * p.W + np - 1) / np); }

template <int R> int fwd_launch(const float *co, float *out, const SampleP &p, hipStream_t s)
{
    hipLaunchKernelGGL((sample_fwd<R, NP_FWD>), dim3(blocks(p, NP_FWD)), dim3(NT), 0, s, co, out, p);
    return launch_status();
}

template <int R> int bwd_launch(const float *co, const float *go, const SampleP &p, hipStream_t s)
{
    hipLaunchKernelGGL((sample_bwd<R, NP_BWD>), dim3(blocks(p, NP_BWD)), dim3(NT), 0, s, co, go, p);
    return launch_status();
}

} // namespace

#define FN2P_DISPATCH(fn, ...)                                                                                                         \
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

int sample_forward(const float *co, float *out, const SampleP &p, hipStream_t s) { FN2P_DISPATCH(fwd_launch, co, out, p, s) }

int sample_backward(const float *co, const float *go, const SampleP &p, hipStream_t s) { FN2P_DISPATCH(bwd_launch, co, go, p, s) }

} // namespace fn2
