// corr_lookup.hip -- CorrLookup: RAFT's on-demand correlation lookup (include/flownet2_hip_lookup.h), gfx950, float32.
//
//   out[b, i D + j, y, x] = scale * sum_{ox,oy} w(ox,oy) * dot(fmap1[b,:,y,x], fmap2[b,:, y0 + j - r + oy, x0 + i - r + ox])
//
// The four corners of neighbouring window taps are the same fmap2 pixels, so everything is organised on the pixel's integer
// GRID of G x G points, G = 2 r + 2: grid point (u, v) is fmap2 pixel (x0 - r + u, y0 - r + v).
//   forward     dots first: g(u,v) = sum_c fmap1[c] * fmap2[c, grid(u,v)], one sequential fp32 chain over ascending c starting
//               at +0; then the four-weight mix of each tap (mix_store).  One lane per (pixel, window row j): it owns grid rows
//               j and j + 1 (2 G accumulators).
//   grad_fmap1  grid weights first: wg(u,v) = scale * (the up to four gO * w terms that meet at the grid point), kept in LDS
//               per pixel; then per channel sum_v (sum_u wg(u,v) * fmap2[c, grid(u,v)]), ascending u inside ascending v.
//   grad_fmap2  the transpose: one float atomic add of wg(u,v) * fmap1[c] per (pixel, channel, grid point) that lies in the
//               image -- G^2 C adds per pixel.  Lanes are consecutive pixels of a row: for a smooth flow one wave-instruction
//               adds to one contiguous row segment of grad_fmap2 (cdna guide, Guideline 12).
// A grid point outside fmap2 is ABSENT: its dot is never mixed in, its weight never multiplied; a pixel with bad coordinates
// (not finite, or |c| >= 2^20) has no grid at all.
//
// General kernels read fmap2 from global memory with clamped indices.  Staged kernels (r <= 4): a workgroup owns a TW x TH
// pixel tile, reduces floor(coords) of its pixels to a bounding box and, if box + halo fits the PW x PH patch, stages that
// fmap2 patch (and, forward, fmap1's tile) per chunk of CK channels in LDS, double-buffered with one barrier per step, the next
// chunk's global loads in flight during the step's arithmetic; every lane then runs the SAME chain over the same operands, so
// the bits are the general kernel's.  A tile whose box does not fit runs the general lane function on a block-uniform branch.
#include "corr_lookup.h"
#include "../../include/flownet2_hip_lookup.h"
#include <limits.h>

namespace fn2 {
namespace {

constexpr int TW = FN2L_TILE_W, TH = FN2L_TILE_H, PW = FN2L_PATCH_W, PH = FN2L_PATCH_H, CK = FN2L_CHUNK;
constexpr int NPIX = TW * TH;
static_assert(NPIX == 64, "a tile is one wave of pixels");
static_assert(PW == 32 && PH == 16, "the staging loops split a patch index with shifts");

struct Pix {
    int x0, y0;     // floor(coords)
    float fx, fy;   // fl(c - floor(c))
    bool ok;        // the pixel has taps: inside the launch's image, coordinates finite and below 2^20
};

__device__ __forceinline__ Pix decode(float cx, float cy, bool inimg)
{
    Pix q;
    q.ok = inimg && (fabsf(cx) < 0x1p20f) && (fabsf(cy) < 0x1p20f);   // NaN compares false; before any float -> int conversion
    const float sx = q.ok ? cx : 0.f, sy = q.ok ? cy : 0.f;
    const float flx = floorf(sx), fly = floorf(sy);
    q.x0 = (int)flx;
    q.y0 = (int)fly;
    q.fx = sx - flx;
    q.fy = sy - fly;
    return q;
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }
__device__ __forceinline__ bool inside(int v, int n) { return (unsigned)v < (unsigned)n; }

// which pixel a lane owns.  TILED: block = one TW x TH tile of one batch item; else a run of NP consecutive pixels (row-major).
template <bool TILED, int NP>
__device__ __forceinline__ void pixel_of(unsigned bid, int lane, const LookupP &P, int &b, int &y, int &x, bool &inimg)
{
    if (TILED) {
        const unsigned nbx = (P.W + TW - 1) / TW, nby = (P.H + TH - 1) / TH;
        const unsigned tx = bid % nbx, t = bid / nbx;
        b = t / nby;
        x = tx * TW + lane % TW;
        y = (t % nby) * TH + lane / TW;
        inimg = x < P.W && y < P.H;
    } else {
        const unsigned HW = (unsigned)P.H * P.W, nblk = (HW + NP - 1) / NP;
        b = bid / nblk;
        const unsigned pi = (bid % nblk) * NP + lane;
        inimg = pi < HW;
        y = inimg ? pi / P.W : 0;
        x = inimg ? pi % P.W : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
// the four-weight mix of window row j from grid rows j (a0) and j + 1 (a1); corners in the order (0,0) (1,0) (0,1) (1,1),
// a sequential sum from +0 over the corners that exist, then * scale
template <int R>
__device__ __forceinline__ void mix_store(float *outp, const float (&a0)[2 * R + 2], const float (&a1)[2 * R + 2], const Pix &q, int j,
                                          size_t HW, int H2, int W2, float scale)
{
    constexpr int D = 2 * R + 1;
    const float ux = 1.f - q.fx, uy = 1.f - q.fy;
    const float w00 = ux * uy, w10 = q.fx * uy, w01 = ux * q.fy, w11 = q.fx * q.fy;
    const bool oky0 = inside(q.y0 + j - R, H2), oky1 = inside(q.y0 + j - R + 1, H2);
    bool okl = inside(q.x0 - R, W2);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const bool okr = inside(q.x0 - R + i + 1, W2);
        float s = 0.f;
        s = (okl && oky0) ? s + w00 * a0[i] : s;
        s = (okr && oky0) ? s + w10 * a0[i + 1] : s;
        s = (okl && oky1) ? s + w01 * a1[i] : s;
        s = (okr && oky1) ? s + w11 * a1[i + 1] : s;
        outp[(size_t)(i * D + j) * HW] = q.ok ? scale * s : 0.f;
        okl = okr;
    }
}

// one (pixel, window row j) from global memory.  f1p = &fmap1[b,0,y,x], f2b = &fmap2[b,0,0,0], outp = &out[b,0,y,x].
// Loads are clamped into the tensor; the dots of absent grid points are discarded by the mix.
template <int R>
__device__ __forceinline__ void fwd_lane_global(const float *f1p, const float *f2b, float *outp, const Pix &q, int j, const LookupP &P)
{
    constexpr int G = 2 * R + 2;
    const size_t HW = (size_t)P.H * P.W, plane2 = (size_t)P.H2 * P.W2;
    int cx[G];
#pragma unroll
    for (int u = 0; u < G; ++u) cx[u] = clampi(q.x0 - R + u, P.W2 - 1);
    const float *row0 = f2b + (size_t)clampi(q.y0 + j - R, P.H2 - 1) * P.W2;
    const float *row1 = f2b + (size_t)clampi(q.y0 + j - R + 1, P.H2 - 1) * P.W2;
    float a0[G], a1[G];
#pragma unroll
    for (int u = 0; u < G; ++u) a0[u] = a1[u] = 0.f;
    if (q.ok) {
#pragma unroll(R <= 4 ? 2 : 1)   // two channels' loads in flight where the registers allow it
        for (int c = 0; c < P.C; ++c) {
            const float a = f1p[(size_t)c * HW];
#pragma unroll
            for (int u = 0; u < G; ++u) {
                a0[u] = a0[u] + a * row0[cx[u]];
                a1[u] = a1[u] + a * row1[cx[u]];
            }
            row0 += plane2;
            row1 += plane2;
        }
    }
    mix_store<R>(outp, a0, a1, q, j, HW, P.H2, P.W2, P.scale);
}

template <int R, int NY>
__global__ __launch_bounds__(64 * NY) void lookup_fwd_general(const float *__restrict__ f1, const float *__restrict__ f2,
                                                              const float *__restrict__ co, float *__restrict__ out, const LookupP P)
{
    constexpr int D = 2 * R + 1;
    int b, y, x;
    bool inimg;
    pixel_of<false, 64>(blockIdx.x, threadIdx.x, P, b, y, x, inimg);
    if (!inimg) return;
    const size_t HW = (size_t)P.H * P.W, pix = (size_t)y * P.W + x;
    const Pix q = decode(co[(size_t)b * 2 * HW + pix], co[((size_t)b * 2 + 1) * HW + pix], true);
    for (int j = threadIdx.y; j < D; j += NY)
        fwd_lane_global<R>(f1 + (size_t)b * P.C * HW + pix, f2 + (size_t)b * P.C * P.H2 * P.W2, out + (size_t)b * D * D * HW + pix, q, j, P);
}

// ---------------------------------------------------------------------------------------------------------------- staging
// the tile's bounding box of floor(coords) over its pixels with taps; false if there is none or box + halo exceeds the patch.
// Two barriers; every thread of the block calls it.  `first` marks one thread per pixel.
template <int R> __device__ __forceinline__ bool tile_box(int *bb, const Pix &q, bool first, int tid, int &bx0, int &by0, int &bw, int &bh)
{
    if (tid == 0) {
        bb[0] = bb[2] = INT_MAX;
        bb[1] = bb[3] = INT_MIN;
    }
    __syncthreads();
    if (first && q.ok) {
        atomicMin(&bb[0], q.x0);
        atomicMax(&bb[1], q.x0);
        atomicMin(&bb[2], q.y0);
        atomicMax(&bb[3], q.y0);
    }
    __syncthreads();
    bx0 = bb[0];
    by0 = bb[2];
    if (bx0 > bb[1]) return false;
    bw = bb[1] - bx0 + 2 * R + 2;   // |floor(c)| <= 2^20: no overflow
    bh = bb[3] - by0 + 2 * R + 2;
    return bw <= PW && bh <= PH;
}

// One channel chunk on its way into LDS: patch[cc][py][px] = fmap2[b, c0 + cc, oy + py, ox + px] (0 outside the image) for
// cc < nc, py < bh, px < bw, and (F1) f1s[cc][lane] = fmap1 at the tile's pixels.  Two phases, so that every global load of a
// step is in flight before the step's arithmetic and lands in LDS after it: stage_load into registers (a fixed count per
// thread over the whole CK x PH x PW index space, predicated; rows are contiguous segments), stage_store into the buffer.
template <int NT, int ROWS> struct StageRegs {   // ROWS: the most patch rows a workgroup of this kernel stages
    static constexpr int NE = (CK * ROWS * PW + NT - 1) / NT, NF = (CK * NPIX + NT - 1) / NT;
    float v[NE], f[NF];
};

template <int NT, int ROWS, bool F1>
__device__ __forceinline__ void stage_load(StageRegs<NT, ROWS> &sr, const float *f2b, const float *f1b, int c0, int nc, int ox, int oy, int bw,
                                           int bh, const LookupP &P, int ty0, int tx0, int tid)
{
    const size_t plane2 = (size_t)P.H2 * P.W2, HW = (size_t)P.H * P.W;
#pragma unroll
    for (int k = 0; k < StageRegs<NT, ROWS>::NE; ++k) {
        const int e = tid + k * NT, cc = e / (ROWS * PW), py = (e / PW) % ROWS, px = e % PW;
        const int gx = ox + px, gy = oy + py;
        float v = 0.f;
        if (cc < nc && py < bh && px < bw && inside(gx, P.W2) && inside(gy, P.H2)) v = f2b[(size_t)(c0 + cc) * plane2 + (size_t)gy * P.W2 + gx];
        sr.v[k] = v;
    }
    if constexpr (F1) {
#pragma unroll
        for (int k = 0; k < StageRegs<NT, ROWS>::NF; ++k) {
            const int e = tid + k * NT, cc = e >> 6, l = e & 63;
            const int x = tx0 + l % TW, y = ty0 + l / TW;
            float v = 0.f;
            if (cc < nc && x < P.W && y < P.H) v = f1b[(size_t)(c0 + cc) * HW + (size_t)y * P.W + x];
            sr.f[k] = v;
        }
    }
}

template <int NT, int ROWS, bool F1>
__device__ __forceinline__ void stage_store(const StageRegs<NT, ROWS> &sr, float *patch, float *f1s, int nc, int bw, int bh, int tid)
{
#pragma unroll
    for (int k = 0; k < StageRegs<NT, ROWS>::NE; ++k) {
        const int e = tid + k * NT, cc = e / (ROWS * PW), py = (e / PW) % ROWS, px = e % PW;
        if (cc < nc && py < bh && px < bw) patch[cc * (PH * PW) + py * PW + px] = sr.v[k];
    }
    if constexpr (F1) {
#pragma unroll
        for (int k = 0; k < StageRegs<NT, ROWS>::NF; ++k) {
            const int e = tid + k * NT;
            if ((e >> 6) < nc) f1s[e] = sr.f[k];
        }
    }
}

// the forward's channel step of one lane: grid rows jl, jl + 1 of the patch against the tile's fmap1 values
template <int G> __device__ __forceinline__ void fwd_step(float (&a0)[G], float (&a1)[G], const float *pt, const float *fa, int cc)
{
    const float a = fa[cc * NPIX];
#pragma unroll
    for (int u = 0; u < G; ++u) {
        a0[u] = a0[u] + a * pt[cc * (PH * PW) + u];
        a1[u] = a1[u] + a * pt[cc * (PH * PW) + PW + u];
    }
}

// JG window rows per workgroup (blockIdx.y picks the group): three times the workgroups of one per tile at r = 4, and a patch
// of span + JG + 1 rows instead of span + 2 r + 2
template <int R, int JG>
__global__ __launch_bounds__(64 * JG) void lookup_fwd_staged(const float *__restrict__ f1, const float *__restrict__ f2,
                                                             const float *__restrict__ co, float *__restrict__ out, const LookupP P)
{
    constexpr int D = 2 * R + 1, G = D + 1, NT = 64 * JG, ROWS = PH - G + JG + 1;
    __shared__ float patch[2][CK * PH * PW];
    __shared__ float f1s[2][CK * NPIX];
    __shared__ int bb[4];
    const int lane = threadIdx.x, jl = threadIdx.y, tid = jl * 64 + lane;
    const int j0 = blockIdx.y * JG, j = j0 + jl;
    const bool active = j < D;   // (the last group may own fewer rows; its spare waves still stage)
    int b, y, x;
    bool inimg;
    pixel_of<true, 64>(blockIdx.x, lane, P, b, y, x, inimg);
    const size_t HW = (size_t)P.H * P.W, pix = (size_t)min(y, P.H - 1) * P.W + min(x, P.W - 1);
    const float *f1b = f1 + (size_t)b * P.C * HW, *f2b = f2 + (size_t)b * P.C * P.H2 * P.W2;
    float *outp = out + (size_t)b * D * D * HW + pix;
    const Pix q = decode(co[(size_t)b * 2 * HW + pix], co[((size_t)b * 2 + 1) * HW + pix], inimg);
    int bx0, by0, bw, bh;
    if (!tile_box<R>(bb, q, jl == 0, tid, bx0, by0, bw, bh)) {   // block-uniform
        if (inimg && active) fwd_lane_global<R>(f1b + pix, f2b, outp, q, j, P);
        return;
    }
    const int ty0 = y - lane / TW, tx0 = x - lane % TW;
    const int ox = bx0 - R, oy = by0 - R + j0, bhg = bh - (2 * R + 2) + JG + 1;   // this group's rows of the box: bhg <= bh <= PH
    // this lane's grid rows j, j + 1 inside the patch; a lane without taps reads the patch's corner (its dots are not stored)
    const int base = q.ok ? (q.y0 - by0 + jl) * PW + (q.x0 - bx0) : 0;
    float a0[G], a1[G];
#pragma unroll
    for (int u = 0; u < G; ++u) a0[u] = a1[u] = 0.f;
    const int steps = (P.C + CK - 1) / CK;
    StageRegs<NT, ROWS> sr;
    stage_load<NT, ROWS, true>(sr, f2b, f1b, 0, min(CK, P.C), ox, oy, bw, bhg, P, ty0, tx0, tid);
    stage_store<NT, ROWS, true>(sr, patch[0], f1s[0], min(CK, P.C), bw, bhg, tid);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int c0 = s * CK, nc = min(CK, P.C - c0), nn = min(CK, P.C - c0 - CK);
        if (s + 1 < steps) stage_load<NT, ROWS, true>(sr, f2b, f1b, c0 + CK, nn, ox, oy, bw, bhg, P, ty0, tx0, tid);
        const float *pt = patch[s & 1] + base, *fa = f1s[s & 1] + lane;
#pragma unroll 2
        for (int cc = 0; cc < nc; ++cc) fwd_step<G>(a0, a1, pt, fa, cc);
        // the other buffer was last read in step s - 1, which ended in a barrier
        if (s + 1 < steps) stage_store<NT, ROWS, true>(sr, patch[(s + 1) & 1], f1s[(s + 1) & 1], nn, bw, bhg, tid);
        __syncthreads();
    }
    if (inimg && active) mix_store<R>(outp, a0, a1, q, j, HW, P.H2, P.W2, P.scale);
}

// ---------------------------------------------------------------------------------------------------------------- backward
// grid weights of NP pixels into LDS, wg[(u G + v) NP + p] = scale * (sum of the gO * w terms that meet at grid point (u,v)):
// terms in the order (i,j,corner) = (u,v,00) (u-1,v,10) (u,v-1,01) (u-1,v-1,11), those whose tap index exists, from +0.
// gop = &gO[b,0,y,x] of pixel p.  A pixel without taps gets zeros.  Thread (p, sub) of NY fills grid points sub, sub + NY, ..
template <int R, int NP, int NY>
__device__ __forceinline__ void grid_weights(float *wg, const float *gop, const Pix &q, size_t HW, float scale, int p, int sub)
{
    constexpr int D = 2 * R + 1, G = D + 1;
    const float ux = 1.f - q.fx, uy = 1.f - q.fy;
    const float w00 = ux * uy, w10 = q.fx * uy, w01 = ux * q.fy, w11 = q.fx * q.fy;
    for (int g = sub; g < G * G; g += NY) {
        const int u = g / G, v = g % G;
        float s = 0.f;
        if (q.ok) {
            if (u < D && v < D) s = s + gop[(size_t)(u * D + v) * HW] * w00;
            if (u >= 1 && v < D) s = s + gop[(size_t)((u - 1) * D + v) * HW] * w10;
            if (u < D && v >= 1) s = s + gop[(size_t)(u * D + v - 1) * HW] * w01;
            if (u >= 1 && v >= 1) s = s + gop[(size_t)((u - 1) * D + v - 1) * HW] * w11;
        }
        wg[g * NP + p] = scale * s;
    }
}

// grad_fmap1 of one (pixel, channel) from global memory: rows ascending v, inside a row ascending u, absent points skipped
template <int R, int NP>
__device__ __forceinline__ float g1_lane_global(const float *wgp, const float *f2c, const Pix &q, const LookupP &P)
{
    constexpr int G = 2 * R + 2;
    int cx[G];
    unsigned okx = 0;
#pragma unroll
    for (int u = 0; u < G; ++u) {
        cx[u] = clampi(q.x0 - R + u, P.W2 - 1);
        okx |= (unsigned)inside(q.x0 - R + u, P.W2) << u;
    }
    float tot = 0.f;
#pragma unroll 1
    for (int v = 0; v < G; ++v) {
        const int gy = q.y0 - R + v;
        const float *row = f2c + (size_t)clampi(gy, P.H2 - 1) * P.W2;
        float rs = 0.f;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const float t = wgp[(u * G + v) * NP] * row[cx[u]];
            rs = ((okx >> u) & 1) ? rs + t : rs;
        }
        tot = (q.ok && inside(gy, P.H2)) ? tot + rs : tot;
    }
    return tot;
}

template <int R, int NP, int NY>
__global__ __launch_bounds__(NP * NY) void lookup_g1_general(const float *__restrict__ f2, const float *__restrict__ co,
                                                             const float *__restrict__ go, float *__restrict__ g1, const LookupP P)
{
    constexpr int D = 2 * R + 1, G = D + 1;
    __shared__ float wg[G * G * NP];
    const int p = threadIdx.x, sub = threadIdx.y;
    int b, y, x;
    bool inimg;
    pixel_of<false, NP>(blockIdx.x, p, P, b, y, x, inimg);
    const size_t HW = (size_t)P.H * P.W, pix = (size_t)y * P.W + x, plane2 = (size_t)P.H2 * P.W2;
    const Pix q = decode(co[(size_t)b * 2 * HW + pix], co[((size_t)b * 2 + 1) * HW + pix], inimg);
    grid_weights<R, NP, NY>(wg, go + (size_t)b * D * D * HW + pix, q, HW, P.scale, p, sub);
    __syncthreads();
    if (!inimg) return;
    for (int c = sub; c < P.C; c += NY)
        g1[((size_t)b * P.C + c) * HW + pix] = g1_lane_global<R, NP>(wg + p, f2 + ((size_t)b * P.C + c) * plane2, q, P);
}

template <int R>
__global__ __launch_bounds__(64 * CK) void lookup_g1_staged(const float *__restrict__ f2, const float *__restrict__ co,
                                                            const float *__restrict__ go, float *__restrict__ g1, const LookupP P)
{
    constexpr int D = 2 * R + 1, G = D + 1, NT = 64 * CK;
    __shared__ float wg[G * G * NPIX];
    __shared__ float patch[2][CK * PH * PW];
    __shared__ int bb[4];
    const int lane = threadIdx.x, sub = threadIdx.y, tid = sub * 64 + lane;
    int b, y, x;
    bool inimg;
    pixel_of<true, 64>(blockIdx.x, lane, P, b, y, x, inimg);
    const size_t HW = (size_t)P.H * P.W, pix = (size_t)min(y, P.H - 1) * P.W + min(x, P.W - 1), plane2 = (size_t)P.H2 * P.W2;
    const float *f2b = f2 + (size_t)b * P.C * plane2;
    float *g1p = g1 + (size_t)b * P.C * HW + pix;
    const Pix q = decode(co[(size_t)b * 2 * HW + pix], co[((size_t)b * 2 + 1) * HW + pix], inimg);
    grid_weights<R, NPIX, CK>(wg, go + (size_t)b * D * D * HW + pix, q, HW, P.scale, lane, sub);
    int bx0, by0, bw, bh;
    const bool fits = tile_box<R>(bb, q, sub == 0, tid, bx0, by0, bw, bh);   // (its barriers also publish wg)
    if (!fits) {   // block-uniform
        if (inimg)
            for (int c = sub; c < P.C; c += CK) g1p[(size_t)c * HW] = g1_lane_global<R, NPIX>(wg + lane, f2b + (size_t)c * plane2, q, P);
        return;
    }
    const int base = q.ok ? (q.y0 - by0) * PW + (q.x0 - bx0) : 0;
    unsigned okx = 0;
#pragma unroll
    for (int u = 0; u < G; ++u) okx |= (unsigned)inside(q.x0 - R + u, P.W2) << u;
    const int steps = (P.C + CK - 1) / CK;
    const int ox = bx0 - R, oy = by0 - R;
    StageRegs<NT, PH> sr;
    stage_load<NT, PH, false>(sr, f2b, nullptr, 0, min(CK, P.C), ox, oy, bw, bh, P, 0, 0, tid);
    stage_store<NT, PH, false>(sr, patch[0], nullptr, min(CK, P.C), bw, bh, tid);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int c0 = s * CK, nc = min(CK, P.C - c0), nn = min(CK, P.C - c0 - CK);
        if (s + 1 < steps) stage_load<NT, PH, false>(sr, f2b, nullptr, c0 + CK, nn, ox, oy, bw, bh, P, 0, 0, tid);
        if (sub < nc) {   // wave-uniform: wave `sub` owns channel c0 + sub of the chunk
            const float *pt = patch[s & 1] + sub * (PH * PW) + base;
            float tot = 0.f;
#pragma unroll 1
            for (int v = 0; v < G; ++v) {
                float rs = 0.f;
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    const float t = wg[(u * G + v) * NPIX + lane] * pt[v * PW + u];
                    rs = ((okx >> u) & 1) ? rs + t : rs;
                }
                tot = (q.ok && inside(q.y0 - R + v, P.H2)) ? tot + rs : tot;
            }
            if (inimg) g1p[(size_t)(c0 + sub) * HW] = tot;
        }
        if (s + 1 < steps) stage_store<NT, PH, false>(sr, patch[(s + 1) & 1], nullptr, nn, bw, bh, tid);
        __syncthreads();
    }
}

// grad_fmap2: g2 was cleared on the stream; every (pixel, channel, grid point inside the image) adds wg * fmap1[c]
template <int R, int NP, int NY>
__global__ __launch_bounds__(NP * NY) void lookup_g2_scatter(const float *__restrict__ f1, const float *__restrict__ co,
                                                             const float *__restrict__ go, float *__restrict__ g2, const LookupP P)
{
    constexpr int D = 2 * R + 1, G = D + 1;
    __shared__ float wg[G * G * NP];
    const int p = threadIdx.x, sub = threadIdx.y;
    int b, y, x;
    bool inimg;
    pixel_of<false, NP>(blockIdx.x, p, P, b, y, x, inimg);
    const size_t HW = (size_t)P.H * P.W, pix = (size_t)y * P.W + x, plane2 = (size_t)P.H2 * P.W2;
    const Pix q = decode(co[(size_t)b * 2 * HW + pix], co[((size_t)b * 2 + 1) * HW + pix], inimg);
    grid_weights<R, NP, NY>(wg, go + (size_t)b * D * D * HW + pix, q, HW, P.scale, p, sub);
    __syncthreads();
    if (!q.ok) return;
    for (int c = sub; c < P.C; c += NY) {
        const float a = f1[((size_t)b * P.C + c) * HW + pix];
        float *dst = g2 + ((size_t)b * P.C + c) * plane2;
#pragma unroll 1
        for (int u = 0; u < G; ++u) {   // (column outside, rows inside: a lane's successive adds go to different rows)
            const int gx = q.x0 - R + u;
            if (!inside(gx, P.W2)) continue;
#pragma unroll
            for (int v = 0; v < G; ++v) {
                const int gy = q.y0 - R + v;
                if (inside(gy, P.H2)) atomicAdd(dst + (size_t)gy * P.W2 + gx, wg[(u * G + v) * NP + p] * a);
            }
        }
    }
}

unsigned blocks_linear(const LookupP &p, int np) { return (unsigned)p.B * (unsigned)(((size_t)p.H * p.W + np - 1) / np); }
unsigned blocks_tiled(const LookupP &p) { return (unsigned)p.B * (unsigned)((p.W + TW - 1) / TW) * (unsigned)((p.H + TH - 1) / TH); }

template <int R> int fwd_general_launch(const float *f1, const float *f2, const float *co, float *out, const LookupP &p, hipStream_t s)
{
    constexpr int D = 2 * R + 1, NY = R <= 4 ? D : (D + 1) / 2;
    hipLaunchKernelGGL((lookup_fwd_general<R, NY>), dim3(blocks_linear(p, 64)), dim3(64, NY), 0, s, f1, f2, co, out, p);
    return launch_status();
}

template <int R> int fwd_staged_launch(const float *f1, const float *f2, const float *co, float *out, const LookupP &p, hipStream_t s)
{
    constexpr int D = 2 * R + 1, JG = R == 0 ? 1 : R == 3 ? 4 : 3;   // row groups of 1 | 3 | 3+2 | 4+3 | 3+3+3
    hipLaunchKernelGGL((lookup_fwd_staged<R, JG>), dim3(blocks_tiled(p), (D + JG - 1) / JG), dim3(64, JG), 0, s, f1, f2, co, out, p);
    return launch_status();
}

template <int R>
int bwd_launch(const float *f1, const float *f2, const float *co, const float *go, float *g1, float *g2, const LookupP &p, bool staged,
               hipStream_t s)
{
    constexpr int NP = R <= 4 ? 64 : 32, NY = 256 / NP;
    int rc = zero_fill_async(g2, (size_t)p.B * p.C * p.H2 * p.W2 * sizeof(float), s);
    if (rc != FN2_OK) return rc;
    if constexpr (R <= FN2L_STAGED_MAX_RADIUS) {
        if (staged) hipLaunchKernelGGL((lookup_g1_staged<R>), dim3(blocks_tiled(p)), dim3(64, CK), 0, s, f2, co, go, g1, p);
        else hipLaunchKernelGGL((lookup_g1_general<R, NP, NY>), dim3(blocks_linear(p, NP)), dim3(NP, NY), 0, s, f2, co, go, g1, p);
    } else {
        hipLaunchKernelGGL((lookup_g1_general<R, NP, NY>), dim3(blocks_linear(p, NP)), dim3(NP, NY), 0, s, f2, co, go, g1, p);
    }
    if ((rc = launch_status()) != FN2_OK) return rc;
    hipLaunchKernelGGL((lookup_g2_scatter<R, NP, NY>), dim3(blocks_linear(p, NP)), dim3(NP, NY), 0, s, f1, co, go, g2, p);
    return launch_status();
}

} // namespace

int lookup_make_params(LookupP &p, int B, int C, int H, int W, int H2, int W2, int radius, float scale)
{
    if (radius < 0 || radius > FN2L_MAX_RADIUS) return FN2_EINVAL;
    if (B < 0 || C < 1 || H < 1 || W < 1 || H2 < 1 || W2 < 1) return FN2_EINVAL;
    p = LookupP{B, C, H, W, H2, W2, radius, scale};
    // planes are indexed with 32-bit integers, blocks with one 32-bit grid dimension
    const long long lim = 0x7fffffffLL;
    if ((long long)H * W > lim || (long long)H2 * W2 > lim) return FN2_EUNSUPPORTED;
    if ((long long)B * (((long long)H * W + 31) / 32) > lim) return FN2_EUNSUPPORTED;
    return FN2_OK;
}

bool lookup_staged_applicable(const LookupP &p) { return p.r <= FN2L_STAGED_MAX_RADIUS; }

#define FN2L_DISPATCH(fn, ...)                                                                                                         \
    switch (p.r) {                                                                                                                     \
    case 0: return fn<0>(__VA_ARGS__);                                                                                                 \
    case 1: return fn<1>(__VA_ARGS__);                                                                                                 \
    case 2: return fn<2>(__VA_ARGS__);                                                                                                 \
    case 3: return fn<3>(__VA_ARGS__);                                                                                                 \
    case 4: return fn<4>(__VA_ARGS__);

int lookup_forward_general(const float *f1, const float *f2, const float *co, float *out, const LookupP &p, hipStream_t s)
{
    FN2L_DISPATCH(fwd_general_launch, f1, f2, co, out, p, s)
    case 5: return fwd_general_launch<5>(f1, f2, co, out, p, s);
    case 6: return fwd_general_launch<6>(f1, f2, co, out, p, s);
    case 7: return fwd_general_launch<7>(f1, f2, co, out, p, s);
    case 8: return fwd_general_launch<8>(f1, f2, co, out, p, s);
    }
    return FN2_EINVAL;
}

int lookup_forward_staged(const float *f1, const float *f2, const float *co, float *out, const LookupP &p, hipStream_t s)
{
    FN2L_DISPATCH(fwd_staged_launch, f1, f2, co, out, p, s)
    }
    return FN2_EUNSUPPORTED;
}

int lookup_backward(const float *f1, const float *f2, const float *co, const float *go, float *g1, float *g2, const LookupP &p,
                    bool staged, hipStream_t s)
{
    FN2L_DISPATCH(bwd_launch, f1, f2, co, go, g1, g2, p, staged, s)
    case 5: return bwd_launch<5>(f1, f2, co, go, g1, g2, p, staged, s);
    case 6: return bwd_launch<6>(f1, f2, co, go, g1, g2, p, staged, s);
    case 7: return bwd_launch<7>(f1, f2, co, go, g1, g2, p, staged, s);
    case 8: return bwd_launch<8>(f1, f2, co, go, g1, g2, p, staged, s);
    }
    return FN2_EINVAL;
}

// AUTO's gate (measured; the header states the points)
bool lookup_staged_pays(const LookupP &p) { return lookup_staged_applicable(p); }

} // namespace fn2
