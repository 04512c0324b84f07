// census.hip -- the ternary census distance (include/flownet2_hip_census.h), forward and backward, gfx950.
// A workgroup of 256 lanes owns a FN2C_TILE_H x FN2C_TILE_W tile of output pixels.  It stages both images' grey tiles with a halo of
// md in LDS (the grey conversion on the way, cells outside the image as 0), the backward also gO' (grad_out inside the border ring,
// 0 elsewhere).  A wave takes four rows of the tile, a lane four vertically adjacent pixels of one column: for every column
// offset dx it reads the 4 + 2 md cells of that column once and uses each for up to four pixels.  The tap loop has no bounds test
// and no branch: the centre offset is evaluated like the others and gives exactly +0 (x = +0, f = +0, d = +0); the loop over dx
// stays rolled, which keeps the forward at 7-8 waves per SIMD and the backward at 4-8 (unrolled: 3 and 2).  Per tap it issues two
// reciprocal square roots and one reciprocal (8 cycles each) among about fifteen plain VALU operations (4 cycles each): at md = 3
// the kernels are bound by vector instruction issue, not by the LDS or by memory; at md = 1 they sit between the copy rate and
// the issue rate.
// The backward is a gather: no atomics, the same bits on every run.  The arithmetic is csrc/census_arith.h, the order the header's.
#include "census.h"
#include "census_arith.h"
#include "../../include/flownet2_hip_census.h"

namespace fn2 {
namespace {

constexpr int NT = 256;
constexpr int TH = FN2C_TILE_H, TW = FN2C_TILE_W;
constexpr int PPT = TH * TW / NT;   // pixels per lane: rows PPT wave .. PPT wave + PPT - 1 of the tile, column = lane
static_assert(TW == FN2_WAVE && TH * TW % NT == 0, "a wave takes whole rows of the tile");

template <int MD> struct Patch {
    static constexpr int PH = TH + 2 * MD, PW = TW + 2 * MD, PP = PW + FN2C_PAD, CELLS = PH * PP, COL = PPT + 2 * MD;
};
static_assert(sizeof(float) * 2 * Patch<3>::CELLS == FN2C_LDS_BYTES(2, 3) && sizeof(float) * 3 * Patch<1>::CELLS == FN2C_LDS_BYTES(3, 1),
              "the header's LDS formula");

struct Tile {
    int n, X0, Y0;
};
__device__ __forceinline__ Tile tile_of(const CensusP &p)
{
    unsigned t = blockIdx.x;
    Tile q;
    q.X0 = (int)(t % (unsigned)p.tiles_x) * TW;
    t /= (unsigned)p.tiles_x;
    q.Y0 = (int)(t % (unsigned)p.tiles_y) * TH;
    q.n = (int)(t / (unsigned)p.tiles_y);
    return q;
}

// One patch cell per lane and step.  The address is clamped into the image, so the load needs no branch; a cell outside the
// image -- for GO also one on the border ring -- is staged as 0.  GO: one plane as it is (grad_out); otherwise the grey of C planes.
template <int MD, bool GO> __device__ __forceinline__ void stage(float *__restrict__ lds, const float *__restrict__ src, const Tile &t, const CensusP &p)
{
    using G = Patch<MD>;
    const long HW = (long)p.H * p.W;
    const float *base = src + (long)t.n * (GO ? 1 : p.C) * HW;
    const int ring = GO ? MD : 0;
    for (int i = threadIdx.x; i < G::PH * G::PW; i += NT) {
        const int ly = i / G::PW, lx = i - ly * G::PW;
        const long gy = (long)t.Y0 - MD + ly, gx = (long)t.X0 - MD + lx;
        const bool inside = gy >= ring && gy < (long)p.H - ring && gx >= ring && gx < (long)p.W - ring;
        const long cy = gy < 0 ? 0 : gy > (long)p.H - 1 ? (long)p.H - 1 : gy, cx = gx < 0 ? 0 : gx > (long)p.W - 1 ? (long)p.W - 1 : gx;
        const long off = cy * p.W + cx;
        float v;
        if (GO) v = base[off];
        else if (p.C == 3) v = census_grey3(base[off], base[HW + off], base[2 * HW + off], p.scale);
        else v = census_grey1(base[off], p.scale);
        lds[ly * G::PP + lx] = inside ? v : 0.f;
    }
}

// the COL cells of column dx that the lane's PPT pixels see
template <int MD> __device__ __forceinline__ void column(float (&v)[Patch<MD>::COL], const float *lds, int cell)
{
#pragma unroll
    for (int i = 0; i < Patch<MD>::COL; ++i) v[i] = lds[cell + i * Patch<MD>::PP];
}

template <int MD>
__global__ __launch_bounds__(NT) void census_fwd(const float *__restrict__ im1, const float *__restrict__ im2, float *__restrict__ out, const CensusP p)
{
    using G = Patch<MD>;
    __shared__ float lds[2 * G::CELLS];   // exactly FN2C_LDS_BYTES(2, MD): one array, no alignment gaps
    float *g1 = lds, *g2 = lds + G::CELLS;
    const Tile t = tile_of(p);
    stage<MD, false>(g1, im1, t, p);
    stage<MD, false>(g2, im2, t, p);
    __syncthreads();

    const int lane = threadIdx.x & (FN2_WAVE - 1), r0 = (threadIdx.x / FN2_WAVE) * PPT;
    const int top = r0 * G::PP + MD + lane;   // patch cell of (row r0 - md, the lane's column)
    float c1[G::COL], c2[G::COL], acc[PPT];
    column<MD>(c1, g1, top);   // the centres are c[MD + j]
    column<MD>(c2, g2, top);
#pragma unroll
    for (int j = 0; j < PPT; ++j) acc[j] = 0.f;
#pragma unroll 1
    for (int dx = -MD; dx <= MD; ++dx) {
        float a[G::COL], b[G::COL];
        column<MD>(a, g1, top + dx);
        column<MD>(b, g2, top + dx);
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            float col = 0.f;
#pragma unroll
            for (int dy = -MD; dy <= MD; ++dy) {
                col = col + census_tap(a[MD + j + dy] - c1[MD + j], b[MD + j + dy] - c2[MD + j]);
            }
            acc[j] = acc[j] + col;
        }
    }

    const int x = t.X0 + lane;
    if (x >= p.W) return;
    float *o = out + (long)t.n * p.H * p.W;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int y = t.Y0 + r0 + j;
        if (y >= p.H) break;
        const bool ring = x < MD || x >= p.W - MD || y < MD || y >= p.H - MD;
        o[(long)y * p.W + x] = ring ? 0.f : p.w * acc[j];
    }
}

// G1 / G2: which gradients are wanted
template <int MD, bool G1, bool G2>
__global__ __launch_bounds__(NT) void census_bwd(const float *__restrict__ im1, const float *__restrict__ im2, const float *__restrict__ go,
                                                 float *__restrict__ gr1, float *__restrict__ gr2, const CensusP p)
{
    using G = Patch<MD>;
    __shared__ float lds[3 * G::CELLS];   // exactly FN2C_LDS_BYTES(3, MD)
    float *g1 = lds, *g2 = lds + G::CELLS, *gs = lds + 2 * G::CELLS;
    const Tile t = tile_of(p);
    stage<MD, false>(g1, im1, t, p);
    stage<MD, false>(g2, im2, t, p);
    stage<MD, true>(gs, go, t, p);
    __syncthreads();

    const int lane = threadIdx.x & (FN2_WAVE - 1), r0 = (threadIdx.x / FN2_WAVE) * PPT;
    const int top = r0 * G::PP + MD + lane;
    float c1[G::COL], c2[G::COL], cs[G::COL], acc1[PPT], acc2[PPT];
    column<MD>(c1, g1, top);
    column<MD>(c2, g2, top);
    column<MD>(cs, gs, top);
#pragma unroll
    for (int j = 0; j < PPT; ++j) acc1[j] = acc2[j] = 0.f;
#pragma unroll 1
    for (int dx = -MD; dx <= MD; ++dx) {
        float a[G::COL], b[G::COL], s[G::COL];
        column<MD>(a, g1, top + dx);
        column<MD>(b, g2, top + dx);
        column<MD>(s, gs, top + dx);
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            float col1 = 0.f, col2 = 0.f;
#pragma unroll
            for (int dy = -MD; dy <= MD; ++dy) {
                const float x1 = c1[MD + j] - a[MD + j + dy], x2 = c2[MD + j] - b[MD + j + dy];
                const float r1 = census_r(x1), r2 = census_r(x2);
                const float tt = (cs[MD + j] + s[MD + j + dy]) * census_dh(x1 * r1 - x2 * r2);
                if (G1) col1 = col1 + tt * census_df_r(r1);
                if (G2) col2 = col2 - tt * census_df_r(r2);
            }
            acc1[j] = acc1[j] + col1;
            acc2[j] = acc2[j] + col2;
        }
    }

    const int x = t.X0 + lane;
    if (x >= p.W) return;
    const long HW = (long)p.H * p.W, plane0 = (long)t.n * p.C * HW;
    const float cw[3] = {p.C == 3 ? FN2C_GREY_R * p.scale : p.scale, FN2C_GREY_G * p.scale, FN2C_GREY_B * p.scale};
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int y = t.Y0 + r0 + j;
        if (y >= p.H) break;
        const long pix = plane0 + (long)y * p.W + x;
        const float a1 = p.w * acc1[j], a2 = p.w * acc2[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c >= p.C) break;
            if (G1) gr1[pix + c * HW] = cw[c] * a1;
            if (G2) gr2[pix + c * HW] = cw[c] * a2;
        }
    }
}

template <int MD> void launch_fwd(const float *im1, const float *im2, float *out, const CensusP &p, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL(census_fwd<MD>, grid, dim3(NT), 0, s, im1, im2, out, p);
}

template <int MD> void launch_bwd(const float *im1, const float *im2, const float *go, float *g1, float *g2, const CensusP &p, dim3 grid, hipStream_t s)
{
    if (g1 && g2) hipLaunchKernelGGL((census_bwd<MD, true, true>), grid, dim3(NT), 0, s, im1, im2, go, g1, g2, p);
    else if (g1) hipLaunchKernelGGL((census_bwd<MD, true, false>), grid, dim3(NT), 0, s, im1, im2, go, g1, g2, p);
    else hipLaunchKernelGGL((census_bwd<MD, false, true>), grid, dim3(NT), 0, s, im1, im2, go, g1, g2, p);
}

} // namespace

int census_make_params(CensusP &p, int N, int C, int H, int W)
{
    if (N < 0 || C < 1 || H < 1 || W < 1) return FN2_EINVAL;
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= (1ull << 31)) return FN2_EUNSUPPORTED;
    const unsigned long long planes = (unsigned long long)N * (unsigned long long)C;
    if (planes >= (1ull << 31) || planes * hw >= (1ull << 48)) return FN2_EUNSUPPORTED;
    const unsigned long long tx = ((unsigned long long)W + TW - 1) / TW, ty = ((unsigned long long)H + TH - 1) / TH;
    if ((unsigned long long)N * tx * ty >= (1ull << 31)) return FN2_EUNSUPPORTED;
    p = CensusP{N, C, H, W, (int)tx, (int)ty, 0, 0.f, 0.f};
    return FN2_OK;
}

int census_set_options(CensusP &p, int md, float scale, int normalize)
{
    if (p.C != 1 && p.C != 3) return FN2_EINVAL;
    if (md < 1 || md > FN2C_MAX_DISTANCE) return FN2_EINVAL;
    if (!(fabsf(scale) <= 3.402823466e38f)) return FN2_EINVAL;   // NaN fails it too
    p.md = md;
    p.scale = scale;
    p.w = normalize ? 1.0f / (float)((2 * md + 1) * (2 * md + 1)) : 1.0f;
    return FN2_OK;
}

int census_forward(const float *im1, const float *im2, float *out, const CensusP &p, hipStream_t s)
{
    const dim3 grid((unsigned)p.N * p.tiles_x * p.tiles_y);
    if (p.md == 1) launch_fwd<1>(im1, im2, out, p, grid, s);
    else if (p.md == 2) launch_fwd<2>(im1, im2, out, p, grid, s);
    else launch_fwd<3>(im1, im2, out, p, grid, s);
    return launch_status();
}

int census_backward(const float *im1, const float *im2, const float *go, float *g1, float *g2, const CensusP &p, hipStream_t s)
{
    const dim3 grid((unsigned)p.N * p.tiles_x * p.tiles_y);
    if (p.md == 1) launch_bwd<1>(im1, im2, go, g1, g2, p, grid, s);
    else if (p.md == 2) launch_bwd<2>(im1, im2, go, g1, g2, p, grid, s);
    else launch_bwd<3>(im1, im2, go, g1, g2, p, grid, s);
    return launch_status();
}

} // namespace fn2
