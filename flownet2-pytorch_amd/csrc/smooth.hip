// smooth.hip -- the edge-aware smoothness term (include/flownet2_hip_smooth.h), forward and backward, gfx950.
// A workgroup of 256 lanes owns a FN2M_TILE_H x FN2M_TILE_W tile of output pixels.  It stages the F flow planes and the C image
// planes of the tile in LDS -- the forward with k more rows below and FN2M_HALO_X more columns to the right, the backward with k
// rows above and below and FN2M_HALO_X columns on either side, plus the two planes of grad_out -- with 16-byte loads where every
// row starts on 16 bytes (W a multiple of 4, the tensors aligned to 16 bytes: FN2M_HALO_X = 4 keeps every patch row on a 16-byte
// boundary), one float at a time otherwise.  The load's address is clamped into the image, so it needs no branch; a cell outside
// the image is staged as 0.  A wave takes four rows of the tile, a lane four vertically adjacent pixels of one column: every LDS
// access of the compute phase is a row segment of 64 consecutive floats, conflict-free at any pitch.  No bounds test in the compute
// phase: whether a cell carries a term is a select at the store (forward) or on grad_out (backward).
// The backward first turns the staged grad_out planes into gO' w in place (one exp2 per cell and direction, image planes read
// from LDS), then every pixel gathers gO' w rho'(d) from the k + 1 cells per direction whose stencil touches it: no atomics, the
// same bits on every run.  The arithmetic is csrc/smooth_arith.h, the orders of summation the header's.
#include "smooth.h"
#include "smooth_arith.h"
#include "../../include/flownet2_hip_smooth.h"

namespace fn2 {
namespace {

constexpr int NT = 256;
constexpr int TH = FN2M_TILE_H, TW = FN2M_TILE_W, HX = FN2M_HALO_X;
constexpr int PPT = TH * TW / NT;   // pixels per lane: rows PPT wave .. PPT wave + PPT - 1 of the tile, column = lane
static_assert(TW == FN2_WAVE && TH * TW % NT == 0, "a wave takes whole rows of the tile");
static_assert(HX % 4 == 0 && HX >= FN2M_MAX_ORDER && TW % 4 == 0, "patch rows start and end on 16 bytes and hold the halo of k");

// rows [Y0 - TOP, Y0 + TH + K), columns [X0 - LEFT, X0 + TW + HX) of the image
template <int K, bool BWD> struct Patch {
    static constexpr int TOP = BWD ? K : 0, LEFT = BWD ? HX : 0;
    static constexpr int PH = TH + TOP + K, PW = TW + LEFT + HX, CELLS = PH * PW;
};
static_assert(sizeof(float) * 5 * Patch<2, false>::CELLS == FN2M_LDS_BYTES(5, 2, 0) && sizeof(float) * 7 * Patch<1, true>::CELLS == FN2M_LDS_BYTES(7, 1, 1),
              "the header's LDS formula");

struct Tile {
    int n, X0, Y0;
};
__device__ __forceinline__ Tile tile_of(const SmoothP &p)
{
    unsigned t = blockIdx.x;
    Tile q;
    q.X0 = (int)(t % (unsigned)p.tiles_x) * TW;
    t /= (unsigned)p.tiles_x;
    q.Y0 = (int)(t % (unsigned)p.tiles_y) * TH;
    q.n = (int)(t / (unsigned)p.tiles_y);
    return q;
}

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : v > hi ? hi : v; }

// P planes of one tensor (N x P x H x W) into P consecutive patch planes.  Four cells (p.vec: W is a multiple of 4 and so is every
// patch column origin, so the four are inside the image together or outside it together) or one cell per lane and step.
template <int P, class G> __device__ __forceinline__ void stage(float *__restrict__ lds, const float *__restrict__ src, const Tile &t, const SmoothP &p)
{
    const long HW = (long)p.H * p.W;
    const float *base = src + (long)t.n * P * HW;
    const long y0 = (long)t.Y0 - G::TOP, x0 = (long)t.X0 - G::LEFT;
    if (p.vec) {
        constexpr int PW4 = G::PW / 4;
        for (int i = threadIdx.x; i < P * G::PH * PW4; i += NT) {
            const int row = i / PW4, l4 = i - row * PW4;   // row = plane PH + patch row
            const int pl = row / G::PH, ly = row - pl * G::PH;
            const long gy = y0 + ly, gx = x0 + 4 * l4;
            const bool inside = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
            const long off = clampl(gy, 0, (long)p.H - 1) * p.W + clampl(gx, 0, (long)p.W - 4);
            float4 v = *reinterpret_cast<const float4 *>(base + pl * HW + off);
            if (!inside) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(lds + row * G::PW + 4 * l4) = v;
        }
    } else {
        for (int i = threadIdx.x; i < P * G::PH * G::PW; i += NT) {
            const int row = i / G::PW, lx = i - row * G::PW;
            const int pl = row / G::PH, ly = row - pl * G::PH;
            const long gy = y0 + ly, gx = x0 + lx;
            const bool inside = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
            const long off = clampl(gy, 0, (long)p.H - 1) * p.W + clampl(gx, 0, (long)p.W - 1);
            const float v = base[pl * HW + off];
            lds[i] = inside ? v : 0.f;
        }
    }
}

// the edge measures of one cell in x and in y from the staged image planes: the channels in ascending order, then the mean
template <int K, int C, int PW, int CELLS> __device__ __forceinline__ void edge_measures(const float *im, int cell, const SmoothP &p, float &ex, float &ey)
{
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v = im[c * CELLS + cell];
        const float ax = smooth_edge_term(im[c * CELLS + cell + K] - v, p.alpha, p.gaussian);
        const float ay = smooth_edge_term(im[c * CELLS + cell + K * PW] - v, p.alpha, p.gaussian);
        ex = c == 0 ? ax : ex + ax;
        ey = c == 0 ? ay : ey + ay;
    }
    if (C == 3) {
        ex = ex * FN2M_THIRD;
        ey = ey * FN2M_THIRD;
    }
}

template <int K, int C, int F>
__global__ __launch_bounds__(NT) void smooth_fwd(const float *__restrict__ flow, const float *__restrict__ image, float *__restrict__ out, const SmoothP p)
{
    using G = Patch<K, false>;
    __shared__ __attribute__((aligned(16))) float lds[(F + C) * G::CELLS];   // exactly FN2M_LDS_BYTES(F + C, K, 0)
    float *fl = lds, *im = lds + F * G::CELLS;
    const Tile t = tile_of(p);
    stage<F, G>(fl, flow, t, p);
    stage<C, G>(im, image, t, p);
    __syncthreads();

    const int lane = threadIdx.x & (FN2_WAVE - 1), r0 = (threadIdx.x / FN2_WAVE) * PPT;
    const int top = r0 * G::PW + lane;   // patch cell of the lane's first pixel
    float wx[PPT], wy[PPT], sx[PPT], sy[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        float ex = 0.f, ey = 0.f;
        edge_measures<K, C, G::PW, G::CELLS>(im, top + j * G::PW, p, ex, ey);
        wx[j] = smooth_weight(ex);
        wy[j] = smooth_weight(ey);
    }
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const float *pl = fl + f * G::CELLS + top;
        float col[PPT + K];
#pragma unroll
        for (int i = 0; i < PPT + K; ++i) col[i] = pl[i * G::PW];
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            float dx, dy;
            if constexpr (K == 1) {
                dx = smooth_d1(col[j], pl[j * G::PW + 1]);
                dy = smooth_d1(col[j], col[j + 1]);
            } else {
                dx = smooth_d2(col[j], pl[j * G::PW + 1], pl[j * G::PW + 2]);
                dy = smooth_d2(col[j], col[j + 1], col[j + K]);
            }
            const float rx = smooth_rho(dx, p.eps2), ry = smooth_rho(dy, p.eps2);
            sx[j] = f == 0 ? rx : sx[j] + rx;
            sy[j] = f == 0 ? ry : sy[j] + ry;
        }
    }

    const int x = t.X0 + lane;
    if (x >= p.W) return;
    const long HW = (long)p.H * p.W;
    float *o = out + (long)t.n * 2 * HW;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int y = t.Y0 + r0 + j;
        if (y >= p.H) break;
        const long pix = (long)y * p.W + x;
        o[pix] = x < p.W - K ? wx[j] * sx[j] : 0.f;
        o[HW + pix] = y < p.H - K ? wy[j] * sy[j] : 0.f;
    }
}

// the gather of one direction from the k + 1 cells reaching a pixel: t0 is the farthest cell (q - k), the last one the pixel's own
template <int K> __device__ __forceinline__ float gather(float t0, float t1, float t2)
{
    return K == 1 ? t0 - t1 : (t0 - 2.0f * t1) + t2;
}

template <int K, int C, int F>
__global__ __launch_bounds__(NT) void smooth_bwd(const float *__restrict__ flow, const float *__restrict__ image, const float *__restrict__ go,
                                                 float *__restrict__ gflow, const SmoothP p)
{
    using G = Patch<K, true>;
    __shared__ __attribute__((aligned(16))) float lds[(F + C + 2) * G::CELLS];   // exactly FN2M_LDS_BYTES(F + C + 2, K, 1)
    float *fl = lds, *im = lds + F * G::CELLS, *gw = lds + (F + C) * G::CELLS;
    const Tile t = tile_of(p);
    stage<F, G>(fl, flow, t, p);
    stage<C, G>(im, image, t, p);
    stage<2, G>(gw, go, t, p);
    __syncthreads();

    // grad_out -> gO' w in place, for the cells the tile's pixels gather from: rows Y0 - K .. Y0 + TH - 1, columns X0 - K .. X0 + TW - 1
    constexpr int RW = TW + K, RH = TH + K;
    for (int i = threadIdx.x; i < RH * RW; i += NT) {
        const int ly = i / RW, lx = G::LEFT - K + (i - ly * RW);
        const int cell = ly * G::PW + lx;
        const long gy = (long)t.Y0 - K + ly, gx = (long)t.X0 - G::LEFT + lx;
        float ex = 0.f, ey = 0.f;
        edge_measures<K, C, G::PW, G::CELLS>(im, cell, p, ex, ey);
        const bool in = gy >= 0 && gx >= 0 && gy < p.H && gx < p.W;
        const bool okx = in && gx < (long)p.W - K, oky = in && gy < (long)p.H - K;
        gw[cell] = (okx ? gw[cell] : 0.f) * smooth_weight(ex);
        gw[G::CELLS + cell] = (oky ? gw[G::CELLS + cell] : 0.f) * smooth_weight(ey);
    }
    __syncthreads();

    const int lane = threadIdx.x & (FN2_WAVE - 1), r0 = (threadIdx.x / FN2_WAVE) * PPT;
    const int centre = (K + r0) * G::PW + G::LEFT + lane;   // patch cell of the lane's first pixel
    const int x = t.X0 + lane;
    const long HW = (long)p.H * p.W;
    float gyw[PPT + K];   // gO' w of the y direction, rows r0 - K .. r0 + PPT - 1 of the lane's column
#pragma unroll
    for (int i = 0; i < PPT + K; ++i) gyw[i] = gw[G::CELLS + centre + (i - K) * G::PW];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const float *pl = fl + f * G::CELLS + centre;
        // y: first differences of the column, rows r0 - K .. r0 + PPT + K - 1; t of the PPT + K cells, each used by up to K + 1 pixels
        float col[PPT + 2 * K], D[PPT + 2 * K - 1], ty[PPT + K];
#pragma unroll
        for (int i = 0; i < PPT + 2 * K; ++i) col[i] = pl[(i - K) * G::PW];
#pragma unroll
        for (int i = 0; i < PPT + 2 * K - 1; ++i) D[i] = col[i + 1] - col[i];
#pragma unroll
        for (int i = 0; i < PPT + K; ++i) ty[i] = gyw[i] * smooth_drho(K == 1 ? D[i] : D[i + 1] - D[i], p.eps2);
        float *g = gflow + ((long)t.n * F + f) * HW;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            // x: the 2 K + 1 values around the pixel, their first differences, t of the K + 1 cells
            float row[2 * K + 1], E[2 * K], tx[K + 1];
#pragma unroll
            for (int i = 0; i < 2 * K + 1; ++i) row[i] = pl[j * G::PW + i - K];
#pragma unroll
            for (int i = 0; i < 2 * K; ++i) E[i] = row[i + 1] - row[i];
#pragma unroll
            for (int m = 0; m <= K; ++m)
                tx[m] = gw[centre + j * G::PW - K + m] * smooth_drho(K == 1 ? E[m] : E[m + 1] - E[m], p.eps2);
            const float gx = gather<K>(tx[0], tx[1], tx[K]), gyv = gather<K>(ty[j], ty[j + 1], ty[j + K]);
            const int y = t.Y0 + r0 + j;
            if (x < p.W && y < p.H) g[(long)y * p.W + x] = gx + gyv;
        }
    }
}

template <int K, int C, int F> int launch(const float *flow, const float *image, const float *go, float *res, const SmoothP &p, dim3 grid, hipStream_t s)
{
    if (go) hipLaunchKernelGGL((smooth_bwd<K, C, F>), grid, dim3(NT), 0, s, flow, image, go, res, p);
    else hipLaunchKernelGGL((smooth_fwd<K, C, F>), grid, dim3(NT), 0, s, flow, image, res, p);
    return launch_status();
}

template <int K, int C> int launch_f(const float *flow, const float *image, const float *go, float *res, const SmoothP &p, dim3 grid, hipStream_t s)
{
    switch (p.F) {
    case 1: return launch<K, C, 1>(flow, image, go, res, p, grid, s);
    case 2: return launch<K, C, 2>(flow, image, go, res, p, grid, s);
    case 3: return launch<K, C, 3>(flow, image, go, res, p, grid, s);
    default: return launch<K, C, 4>(flow, image, go, res, p, grid, s);
    }
}

// go == nullptr: the forward
int dispatch(const float *flow, const float *image, const float *go, float *res, SmoothP &p, hipStream_t s)
{
    p.vec = p.W % 4 == 0 && aligned(flow, 16) && aligned(image, 16) && (!go || aligned(go, 16));
    const dim3 grid((unsigned)p.N * p.tiles_x * p.tiles_y);
    if (p.order == 1) return p.C == 1 ? launch_f<1, 1>(flow, image, go, res, p, grid, s) : launch_f<1, 3>(flow, image, go, res, p, grid, s);
    return p.C == 1 ? launch_f<2, 1>(flow, image, go, res, p, grid, s) : launch_f<2, 3>(flow, image, go, res, p, grid, s);
}

} // namespace

int smooth_make_params(SmoothP &p, int N, int F, int C, int H, int W)
{
    if (N < 0 || F < 1 || C < 1 || H < 1 || W < 1) return FN2_EINVAL;
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= (1ull << 31)) return FN2_EUNSUPPORTED;
    const unsigned long long most = (unsigned long long)(F > C ? F : C) > 2 ? (unsigned long long)(F > C ? F : C) : 2;   // the widest tensor's planes per sample
    const unsigned long long planes = (unsigned long long)N * most;
    if (planes >= (1ull << 31) || planes * hw >= (1ull << 48)) return FN2_EUNSUPPORTED;
    const unsigned long long tx = ((unsigned long long)W + TW - 1) / TW, ty = ((unsigned long long)H + TH - 1) / TH;
    if ((unsigned long long)N * tx * ty >= (1ull << 31)) return FN2_EUNSUPPORTED;
    p = SmoothP{N, F, C, H, W, (int)tx, (int)ty, 0, 0, 0, 0.f, 0.f};
    return FN2_OK;
}

int smooth_set_options(SmoothP &p, int order, int edge, float alpha, float eps)
{
    if (p.C != 1 && p.C != 3) return FN2_EINVAL;
    if (p.F > FN2M_MAX_FLOW_CHANNELS) return FN2_EINVAL;
    if (order < 1 || order > FN2M_MAX_ORDER) return FN2_EINVAL;
    if (edge != FN2M_EDGE_EXPONENTIAL && edge != FN2M_EDGE_GAUSSIAN) return FN2_EINVAL;
    if (!(alpha >= 0.f && alpha <= 3.402823466e38f) || !(eps >= 0.f && eps <= 3.402823466e38f)) return FN2_EINVAL;   // NaN fails it too
    p.order = order;
    p.gaussian = edge == FN2M_EDGE_GAUSSIAN;
    p.alpha = alpha;
    p.eps2 = eps * eps;
    return FN2_OK;
}

int smooth_forward(const float *flow, const float *image, float *out, SmoothP p, hipStream_t s)
{
    return dispatch(flow, image, nullptr, out, p, s);
}

int smooth_backward(const float *flow, const float *image, const float *go, float *gflow, SmoothP p, hipStream_t s)
{
    return dispatch(flow, image, go, gflow, p, s);
}

} // namespace fn2
