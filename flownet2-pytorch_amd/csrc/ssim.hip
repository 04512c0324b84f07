// ssim.hip -- the structural-similarity distance (include/staging/flownet2_hip_ssim.h), forward and backward, gfx950.
// A workgroup of 256 lanes owns a FN2I_TILE_H x FN2I_TILE_W tile of one plane.  It stages the tile of both images in LDS -- the
// forward with md rows above and below and FN2I_HALO_X columns on either side, the backward with twice that -- with 16-byte loads
// where every row starts on 16 bytes (W a multiple of 4, the tensors aligned to 16 bytes), one float at a time otherwise.  The
// load's address is reflected (reflect mode) or clamped (zero mode: a cell outside the image is staged as 0) into the image, so
// it needs no branch.  A wave takes four rows of the tile, a lane four vertically adjacent pixels of one column: every LDS access
// of the compute phases is a row segment of consecutive floats.
// The window statistics are one function for both directions (window_stats): the mean, then the second moments about it, the
// header's order.  The backward recomputes them for the windows within md of the tile, leaves six coefficient maps in LDS and every
// pixel gathers from the k x k maps' cells around it: no atomics, the same bits on every run.
#include "ssim.h"
#include "../../include/staging/flownet2_hip_ssim.h"

namespace fn2 {
namespace {

constexpr int NT = 256;
constexpr int TH = FN2I_TILE_H, TW = FN2I_TILE_W, HX = FN2I_HALO_X, MP = FN2I_MAP_PITCH;
constexpr int PPT = TH * TW / NT;   // pixels per lane: rows PPT wave .. PPT wave + PPT - 1 of the tile, column = lane
static_assert(TW == FN2_WAVE && TH * TW % NT == 0, "a wave takes whole rows of the tile");
static_assert(HX % 4 == 0 && HX >= FN2I_MAX_DISTANCE && TW % 4 == 0, "patch rows start and end on 16 bytes and hold the halo of md");
static_assert(MP >= TW + 2 * FN2I_MAX_DISTANCE, "a map row holds the windows within md of the tile");

// rows [Y0 - R MD, Y0 + TH + R MD), columns [X0 - R HX, X0 + TW + R HX) of the image: R = 1 forward, 2 backward
template <int MD, int R> struct Patch {
    static constexpr int TOP = R * MD, LEFT = R * HX;
    static constexpr int PH = TH + 2 * TOP, PW = TW + 2 * LEFT, CELLS = PH * PW;
};
static_assert(sizeof(float) * 2 * Patch<3, 1>::CELLS == FN2I_LDS_FWD(3) &&
                  sizeof(float) * (2 * Patch<2, 2>::CELLS + 6 * (TH + 2 * 2) * MP) == FN2I_LDS_BWD(2),
              "the header's LDS formulas");

struct Tile {
    long plane;
    int X0, Y0;
};
__device__ __forceinline__ Tile tile_of(const SsimP &p)
{
    unsigned t = blockIdx.x;
    Tile q;
    q.X0 = (int)(t % (unsigned)p.tiles_x) * TW;
    t /= (unsigned)p.tiles_x;
    q.Y0 = (int)(t % (unsigned)p.tiles_y) * TH;
    q.plane = (long)(t / (unsigned)p.tiles_y);
    return q;
}

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return v < lo ? lo : v > hi ? hi : v; }
// the image index an extended position reads.  One reflection is all there is: ssim_set_options refuses reflect mode unless
// H > md and W > md, so every position a valid window reads (at most md outside the image) reflects into it.  The kernels depend
// on that check.  Positions further out are staged for the patch's shape only, no valid window reads them, and the clamp keeps
// their loads inside the image.
__device__ __forceinline__ long reflectl(long i, long n) { return clampl(i < 0 ? -i : i > n - 1 ? 2 * (n - 1) - i : i, 0, n - 1); }

// One plane into one patch.  Four cells (p.vec: W is a multiple of 4 and so is every patch column origin, so the four are inside
// the image together or outside it together) or one cell per lane and step.
template <class G, bool REFLECT> __device__ __forceinline__ void stage(float *__restrict__ lds, const float *__restrict__ src, const Tile &t, const SsimP &p)
{
    const long y0 = (long)t.Y0 - G::TOP, x0 = (long)t.X0 - G::LEFT;
    if (p.vec) {
        constexpr int PW4 = G::PW / 4;
        for (int i = threadIdx.x; i < G::PH * PW4; i += NT) {
            const int ly = i / PW4, l4 = i - ly * PW4;
            const long gy = y0 + ly, gx = x0 + 4 * l4;
            const bool xin = gx >= 0 && gx < p.W;
            float4 v;
            if (REFLECT) {
                const float *row = src + reflectl(gy, p.H) * p.W;
                if (xin) v = *reinterpret_cast<const float4 *>(row + gx);
                else v = make_float4(row[reflectl(gx, p.W)], row[reflectl(gx + 1, p.W)], row[reflectl(gx + 2, p.W)], row[reflectl(gx + 3, p.W)]);
            } else {
                const long off = clampl(gy, 0, (long)p.H - 1) * p.W + clampl(gx, 0, (long)p.W - 4);
                v = *reinterpret_cast<const float4 *>(src + off);
                if (!(xin && gy >= 0 && gy < p.H)) v = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            *reinterpret_cast<float4 *>(lds + ly * G::PW + 4 * l4) = v;
        }
    } else {
        for (int i = threadIdx.x; i < G::CELLS; i += NT) {
            const int ly = i / G::PW, lx = i - ly * G::PW;
            const long gy = y0 + ly, gx = x0 + lx;
            if (REFLECT) {
                lds[i] = src[reflectl(gy, p.H) * p.W + reflectl(gx, p.W)];
            } else {
                const bool inside = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
                const float v = src[clampl(gy, 0, (long)p.H - 1) * p.W + clampl(gx, 0, (long)p.W - 1)];
                lds[i] = inside ? v : 0.f;
            }
        }
    }
}

struct Stats {
    float mx, my, A1, A2, B1, B2, S, d;   // d: (1 - S) / 2 before the clamp
};

// the statistics of the k x k window whose first (top left) cell is `first`: the header's arithmetic, in its order
template <int MD> __device__ __forceinline__ Stats window_stats(const float *xs, const float *ys, int first, int pitch, float c1, float c2)
{
    constexpr int K = 2 * MD + 1, NN = K * K;
    constexpr float R = 1.0f / (float)NN;
    float xv[NN], yv[NN];
#pragma unroll
    for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            xv[dy * K + dx] = xs[first + dy * pitch + dx];
            yv[dy * K + dx] = ys[first + dy * pitch + dx];
        }
    float ax = xv[0], ay = yv[0];
#pragma unroll
    for (int i = 1; i < NN; ++i) {
        ax += xv[i];
        ay += yv[i];
    }
    Stats s;
    s.mx = ax * R;
    s.my = ay * R;
    float qx = 0.f, qy = 0.f, qxy = 0.f;
#pragma unroll
    for (int i = 0; i < NN; ++i) {
        const float ex = xv[i] - s.mx, ey = yv[i] - s.my;
        qx = i == 0 ? ex * ex : qx + ex * ex;
        qy = i == 0 ? ey * ey : qy + ey * ey;
        qxy = i == 0 ? ex * ey : qxy + ex * ey;
    }
    const float sx = qx * R, sy = qy * R, sxy = qxy * R;
    s.A1 = (2.0f * s.mx) * s.my + c1;
    s.A2 = 2.0f * sxy + c2;
    s.B1 = (s.mx * s.mx + s.my * s.my) + c1;
    s.B2 = (sx + sy) + c2;
    s.S = (s.A1 * s.A2) / (s.B1 * s.B2);
    s.d = (1.0f - s.S) * 0.5f;
    return s;
}

// whether the window centred at (y, x) exists: inside the image, and in zero mode not on the ring
template <int MD, bool REFLECT> __device__ __forceinline__ bool window_valid(long y, long x, const SsimP &p)
{
    constexpr long M = REFLECT ? 0 : MD;
    return y >= M && y < (long)p.H - M && x >= M && x < (long)p.W - M;
}

template <int MD, bool REFLECT>
__global__ __launch_bounds__(NT) void ssim_fwd(const float *__restrict__ im1, const float *__restrict__ im2, float *__restrict__ out, const SsimP p)
{
    using G = Patch<MD, 1>;
    __shared__ __attribute__((aligned(16))) float lds[2 * G::CELLS];   // exactly FN2I_LDS_FWD(MD)
    float *xs = lds, *ys = lds + G::CELLS;
    const Tile t = tile_of(p);
    const long HW = (long)p.H * p.W;
    stage<G, REFLECT>(xs, im1 + t.plane * HW, t, p);
    stage<G, REFLECT>(ys, im2 + t.plane * HW, t, p);
    __syncthreads();

    const int lane = threadIdx.x & (FN2_WAVE - 1), r0 = (threadIdx.x / FN2_WAVE) * PPT;
    const long x = (long)t.X0 + lane;
    if (x >= p.W) return;
    float *o = out + t.plane * HW;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const long y = (long)t.Y0 + r0 + j;
        if (y >= p.H) break;
        float v = 0.f;
        if (window_valid<MD, REFLECT>(y, x, p)) {
            const Stats s = window_stats<MD>(xs, ys, (r0 + j) * G::PW + (G::LEFT - MD + lane), G::PW, p.c1, p.c2);
            v = fminf(fmaxf(s.d, 0.f), 1.f);
        }
        o[y * p.W + x] = v;
    }
}

// how many of the extended positions that read image index q lie inside the window centred at c, along one axis of length n
template <int MD> __device__ __forceinline__ int fold_weight(long q, long c, long n)
{
    int w = 1;   // q itself: the gather visits only windows that contain it
    const long lo = -q, hi = 2 * (n - 1) - q;
    if (q >= 1 && q <= MD && lo - c >= -MD && lo - c <= MD) ++w;
    if (n - 1 - q >= 1 && n - 1 - q <= MD && hi - c >= -MD && hi - c <= MD) ++w;
    return w;
}

template <int MD, bool REFLECT>
__global__ __launch_bounds__(NT) void ssim_bwd(const float *__restrict__ im1, const float *__restrict__ im2, const float *__restrict__ go,
                                               float *__restrict__ g1, float *__restrict__ g2, const SsimP p)
{
    using G = Patch<MD, 2>;
    constexpr int K = 2 * MD + 1, MH = TH + 2 * MD, MW = TW + 2 * MD, MCELLS = MH * MP;
    constexpr float R = 1.0f / (float)(K * K);
    __shared__ __attribute__((aligned(16))) float lds[2 * G::CELLS + 6 * MCELLS];   // exactly FN2I_LDS_BWD(MD)
    float *xs = lds, *ys = lds + G::CELLS, *maps = lds + 2 * G::CELLS;
    float *mMx = maps, *mMy = maps + MCELLS, *mA = maps + 2 * MCELLS, *mB = maps + 3 * MCELLS, *mmx = maps + 4 * MCELLS, *mmy = maps + 5 * MCELLS;
    const Tile t = tile_of(p);
    const long HW = (long)p.H * p.W;
    stage<G, REFLECT>(xs, im1 + t.plane * HW, t, p);
    stage<G, REFLECT>(ys, im2 + t.plane * HW, t, p);
    __syncthreads();

    // the maps of the windows centred at rows Y0 - MD .. Y0 + TH + MD - 1, columns X0 - MD .. X0 + TW + MD - 1; +0 where there is none
    const float *gop = go + t.plane * HW;
    for (int i = threadIdx.x; i < MH * MW; i += NT) {
        const int ly = i / MW, lx = i - ly * MW;
        const long py = (long)t.Y0 - MD + ly, px = (long)t.X0 - MD + lx;
        float Mx = 0.f, My = 0.f, A = 0.f, B = 0.f, mx = 0.f, my = 0.f;
        if (window_valid<MD, REFLECT>(py, px, p)) {
            const Stats s = window_stats<MD>(xs, ys, ly * G::PW + (G::LEFT - 2 * MD + lx), G::PW, p.c1, p.c2);
            const bool pass = s.d >= 0.f && s.d <= 1.f;
            const float gp = pass ? -0.5f * gop[py * p.W + px] : 0.f;
            const float E = 1.0f / (s.B1 * s.B2);
            const float Dsxy = (2.0f * s.A1) * E, Ds = -(s.S / s.B2);
            const float Dmx = ((2.0f * s.my) * s.A2) * E - ((2.0f * s.mx) * s.S) / s.B1;
            const float Dmy = ((2.0f * s.mx) * s.A2) * E - ((2.0f * s.my) * s.S) / s.B1;
            const float gn = gp * R;
            Mx = gn * Dmx;
            My = gn * Dmy;
            A = gn * (2.0f * Ds);
            B = gn * Dsxy;
            mx = s.mx;
            my = s.my;
        }
        const int cell = ly * MP + lx;
        mMx[cell] = Mx;
        mMy[cell] = My;
        mA[cell] = A;
        mB[cell] = B;
        mmx[cell] = mx;
        mmy[cell] = my;
    }
    __syncthreads();

    // The lane's PPT pixels share a column: a maps' cell of row i serves the pixels j with 0 <= i - j < K, so it is read once for
    // all of them.  For every pixel the taps still arrive in row-major order of the windows: the header's order, the same bits.
    const int lane = threadIdx.x & (FN2_WAVE - 1), r0 = (threadIdx.x / FN2_WAVE) * PPT;
    const long x = (long)t.X0 + lane, y0 = (long)t.Y0 + r0;
    if (x >= p.W) return;
    float xq[PPT], yq[PPT], gx[PPT], gy[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int centre = (G::TOP + r0 + j) * G::PW + G::LEFT + lane;
        xq[j] = xs[centre];
        yq[j] = ys[centre];
        gx[j] = gy[j] = 0.f;
    }
    int wx[K];
#pragma unroll
    for (int dx = 0; dx < K; ++dx) wx[dx] = REFLECT ? fold_weight<MD>(x, x + dx - MD, p.W) : 1;
#pragma unroll 1   // (unrolled, the rows' loads are hoisted together and the registers run out)
    for (int i = 0; i < PPT + K - 1; ++i) {   // the maps' row r0 + i: the windows centred at row y0 + i - MD
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
            const int cell = (r0 + i) * MP + lane + dx;   // the window centred at (y0 + i - MD, x + dx - MD)
            const float Mx = mMx[cell], My = mMy[cell], A = mA[cell], B = mB[cell], mx = mmx[cell], my = mmy[cell];
#pragma unroll
            for (int j = 0; j < PPT; ++j) {
                const int dy = i - j;
                if (dy < 0 || dy >= K) continue;
                const float ex = xq[j] - mx, ey = yq[j] - my;
                float tx = (Mx + A * ex) + B * ey;
                float ty = (My + A * ey) + B * ex;
                if (REFLECT) {
                    const float w = (float)(fold_weight<MD>(y0 + j, y0 + i - MD, p.H) * wx[dx]);
                    tx = w * tx;
                    ty = w * ty;
                }
                gx[j] = dy == 0 && dx == 0 ? tx : gx[j] + tx;
                gy[j] = dy == 0 && dx == 0 ? ty : gy[j] + ty;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const long y = y0 + j;
        if (y >= p.H) break;
        if (g1) g1[t.plane * HW + y * p.W + x] = gx[j];
        if (g2) g2[t.plane * HW + y * p.W + x] = gy[j];
    }
}

template <int MD, bool REFLECT> int launch(const float *im1, const float *im2, const float *go, float *r1, float *r2, const SsimP &p, dim3 grid, hipStream_t s)
{
    if (go) hipLaunchKernelGGL((ssim_bwd<MD, REFLECT>), grid, dim3(NT), 0, s, im1, im2, go, r1, r2, p);
    else hipLaunchKernelGGL((ssim_fwd<MD, REFLECT>), grid, dim3(NT), 0, s, im1, im2, r1, p);
    return launch_status();
}

template <int MD> int launch_b(const float *im1, const float *im2, const float *go, float *r1, float *r2, const SsimP &p, dim3 grid, hipStream_t s)
{
    return p.reflect ? launch<MD, true>(im1, im2, go, r1, r2, p, grid, s) : launch<MD, false>(im1, im2, go, r1, r2, p, grid, s);
}

// go == nullptr: the forward, r1 its output
int dispatch(const float *im1, const float *im2, const float *go, float *r1, float *r2, SsimP &p, hipStream_t s)
{
    p.vec = p.W % 4 == 0 && aligned(im1, 16) && aligned(im2, 16);
    const dim3 grid((unsigned)p.planes * p.tiles_x * p.tiles_y);
    switch (p.md) {
    case 1: return launch_b<1>(im1, im2, go, r1, r2, p, grid, s);
    case 2: return launch_b<2>(im1, im2, go, r1, r2, p, grid, s);
    default: return launch_b<3>(im1, im2, go, r1, r2, p, grid, s);
    }
}

} // namespace

int ssim_make_params(SsimP &p, int N, int C, int H, int W)
{
    if (N < 0 || C < 1 || H < 1 || W < 1) return FN2_EINVAL;
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= (1ull << 31)) return FN2_EUNSUPPORTED;
    const unsigned long long planes = (unsigned long long)N * (unsigned long long)C;
    if (planes >= (1ull << 31) || planes * hw >= (1ull << 48)) return FN2_EUNSUPPORTED;
    const unsigned long long tx = ((unsigned long long)W + TW - 1) / TW, ty = ((unsigned long long)H + TH - 1) / TH;
    if (planes * tx * ty >= (1ull << 31)) return FN2_EUNSUPPORTED;
    p = SsimP{(int)planes, H, W, (int)tx, (int)ty, 0, 0, 0, 0.f, 0.f};
    return FN2_OK;
}

int ssim_set_options(SsimP &p, int md, float c1, float c2, int border)
{
    if (md < 1 || md > FN2I_MAX_DISTANCE) return FN2_EINVAL;
    if (!(c1 > 0.f && c1 <= 3.402823466e38f) || !(c2 > 0.f && c2 <= 3.402823466e38f)) return FN2_EINVAL;   // NaN fails it too
    if (border != FN2I_BORDER_ZERO && border != FN2I_BORDER_REFLECT) return FN2_EINVAL;
    if (border == FN2I_BORDER_REFLECT && (p.H <= md || p.W <= md)) return FN2_EINVAL;   // reflectl and fold_weight rely on this: one reflection
    p.md = md;
    p.reflect = border == FN2I_BORDER_REFLECT;
    p.c1 = c1;
    p.c2 = c2;
    return FN2_OK;
}

int ssim_forward(const float *im1, const float *im2, float *out, SsimP p, hipStream_t s)
{
    return dispatch(im1, im2, nullptr, out, nullptr, p, s);
}

int ssim_backward(const float *im1, const float *im2, const float *go, float *g1, float *g2, SsimP p, hipStream_t s)
{
    return dispatch(im1, im2, go, g1, g2, p, s);
}

} // namespace fn2
