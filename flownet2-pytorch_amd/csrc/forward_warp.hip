// forward_warp.hip -- ForwardWarp (include/flownet2_hip_splat.h): forward flow splatting, forward and backward, gfx950.
// The forward is a scatter: every source pixel adds to the four cells around where its flow takes it.  Three forms:
//   general        one lane per source pixel, lanes along x, a loop over channels, one float atomic per tap inside the image
//   tiled          a workgroup sums the contributions of a FN2S_TILE_H x FN2S_TILE_W tile of source pixels in an LDS patch (tile
//                  plus FN2S_HALO on every side, fp64 cells, moved by the rounded flow of the tile's centre pixel) and flushes it with
//                  one atomic per touched cell, in contiguous row segments; what lands outside the patch goes straight to memory
//   deterministic  the general form adding int64 fixed-point values to a workspace, and a conversion pass
// The backward is a gather without atomics.  The tap computation is csrc/splat_taps.h, the arithmetic order the header's.
#include "forward_warp.h"
#include "splat_fixed.h"
#include "splat_taps.h"
#include "../../include/flownet2_hip_splat.h"

namespace fn2 {
namespace {

constexpr int NT = 256;
constexpr int TH = FN2S_TILE_H, TW = FN2S_TILE_W, HALO = FN2S_HALO, CG = FN2S_CHANNEL_GROUP;
constexpr int PH = TH + 2 * HALO, PW = TW + 2 * HALO, PP = PW + 1;   // patch rows, columns, pitch (+1: rows on different banks)
constexpr int PPT = TH * TW / NT;
static_assert(TW == FN2_WAVE && TH * TW % NT == 0, "a wave takes one row of the tile");

enum { A00 = 1, A01 = 2, A10 = 4, A11 = 8, IN_PATCH = 16 };

// which taps add to global memory: inside the image and of non-zero weight
__device__ __forceinline__ int taps_inside(const SplatTaps &t, int W, int H)
{
    const bool x0 = t.x0 >= 0, x1 = t.x0 + 1 < W, y0 = t.y0 >= 0, y1 = t.y0 + 1 < H;
    return (y0 && x0 && t.w00 != 0.f ? A00 : 0) | (y0 && x1 && t.w01 != 0.f ? A01 : 0) | (y1 && x0 && t.w10 != 0.f ? A10 : 0) |
           (y1 && x1 && t.w11 != 0.f ? A11 : 0);
}

// the source pixel of a one-lane-per-pixel kernel: workgroup = (batch item, 256-pixel chunk of the plane)
struct Pixel {
    int b, x, y;
    long pix;
    bool live;
};
__device__ __forceinline__ Pixel pixel(const SplatP &p)
{
    Pixel q;
    q.b = (int)(blockIdx.x / (unsigned)p.chunks);
    q.pix = (long)(blockIdx.x % (unsigned)p.chunks) * NT + threadIdx.x;
    q.live = q.pix < (long)p.H * p.W;
    q.y = q.live ? (int)((unsigned)q.pix / (unsigned)p.W) : 0;   // a live pixel's index is below 2^31
    q.x = q.live ? (int)((unsigned)q.pix % (unsigned)p.W) : 0;
    return q;
}

// DET: int64 fixed-point adds into the workspace's planes instead of float adds into out
template <bool DET>
__global__ __launch_bounds__(NT) void splat_fwd_general(const float *__restrict__ in, const float *__restrict__ flow, float *__restrict__ out,
                                                        unsigned long long *__restrict__ acc, const unsigned *__restrict__ pmax, const SplatP p)
{
    const Pixel q = pixel(p);
    if (!q.live) return;
    const long HW = (long)p.H * p.W;
    const float *fl = flow + (long)q.b * 2 * HW;
    const SplatTaps t = splat_taps(splat_pos(q.x, fl[q.pix]), splat_pos(q.y, fl[HW + q.pix]), p.W, p.H);
    if (!t.valid) return;
    const int a = taps_inside(t, p.W, p.H);
    if (!a) return;
    const long base = (long)t.y0 * p.W + t.x0;   // read only together with a tap inside the image
    for (int c = 0; c < p.C; ++c) {
        const long plane = (long)q.b * p.C + c;
        const float v = in[plane * HW + q.pix];
        if constexpr (DET) {
            int s;
            if (splat_scale(pmax[plane], p.K, s) != SPLAT_PLANE_FINITE) continue;
            unsigned long long *A = acc + plane * HW;
            if (a & A00) atomicAdd(A + base, splat_q(t.w00 * v, s));
            if (a & A01) atomicAdd(A + base + 1, splat_q(t.w01 * v, s));
            if (a & A10) atomicAdd(A + base + p.W, splat_q(t.w10 * v, s));
            if (a & A11) atomicAdd(A + base + p.W + 1, splat_q(t.w11 * v, s));
        } else {
            float *O = out + plane * HW;
            if (a & A00) unsafeAtomicAdd(O + base, t.w00 * v);
            if (a & A01) unsafeAtomicAdd(O + base + 1, t.w01 * v);
            if (a & A10) unsafeAtomicAdd(O + base + p.W, t.w10 * v);
            if (a & A11) unsafeAtomicAdd(O + base + p.W + 1, t.w11 * v);
        }
    }
}

// fp64 LDS cell += the fp32 contribution (widened exactly): ds_add_f64 without a return value.  The cell is rounded to fp32 once, at
// the flush.  fp32 cells with ds_add_f32 measured 2-2.5 times the kernel's time (76 against 28 us at 8 x 32 x 96 x 128 with a
// zero flow): the LDS float add is what bounded it.
__device__ __forceinline__ void lds_add(double *cell, float v)
{
    __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double *)cell, (double)v);
}

__global__ __launch_bounds__(NT) void splat_fwd_tiled(const float *__restrict__ in, const float *__restrict__ flow, float *__restrict__ out,
                                                      const SplatP p)
{
    __shared__ double patch[CG][PH * PP];
    const int tid = threadIdx.x;
    // workgroup = (tile, run of p.groups_per_wg channel groups): a plane of few tiles with many channels still fills the chip
    unsigned t = blockIdx.x / (unsigned)p.group_runs;
    const long c_first = (long)(blockIdx.x % (unsigned)p.group_runs) * p.groups_per_wg * CG;
    const long c_end = min((long)p.C, c_first + (long)p.groups_per_wg * CG);
    const int X0 = (int)(t % (unsigned)p.tiles_x) * TW;
    t /= (unsigned)p.tiles_x;
    const int Y0 = (int)(t % (unsigned)p.tiles_y) * TH;
    const int b = (int)(t / (unsigned)p.tiles_y);
    const long HW = (long)p.H * p.W;
    const float *fl = flow + (long)b * 2 * HW;

    // the patch's place: the tile, a halo around it, moved by the rounded flow of the tile's centre pixel where that is a
    // number below 10^6 (the same for every lane; any other value leaves the patch on the tile)
    const long cpix = (long)min(Y0 + TH / 2, p.H - 1) * p.W + min(X0 + TW / 2, p.W - 1);
    const float cfx = fl[cpix], cfy = fl[HW + cpix];
    const long px0 = (long)X0 - HALO + (fabsf(cfx) < 1.0e6f ? (int)rintf(cfx) : 0);
    const long py0 = (long)Y0 - HALO + (fabsf(cfy) < 1.0e6f ? (int)rintf(cfy) : 0);

    float w[PPT][4];
    int base[PPT], flags[PPT];
    long pix[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int idx = tid + NT * k;
        const int x = X0 + idx % TW, y = Y0 + idx / TW;
        w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0.f;
        base[k] = flags[k] = 0;
        pix[k] = -1;
        if (x >= p.W || y >= p.H) continue;
        pix[k] = (long)y * p.W + x;
        const SplatTaps s = splat_taps(splat_pos(x, fl[pix[k]]), splat_pos(y, fl[HW + pix[k]]), p.W, p.H);
        if (!s.valid) continue;
        w[k][0] = s.w00; w[k][1] = s.w01; w[k][2] = s.w10; w[k][3] = s.w11;
        const long lx = (long)s.x0 - px0, ly = (long)s.y0 - py0;
        if (lx >= 0 && lx <= PW - 2 && ly >= 0 && ly <= PH - 2) {   // all four taps in the patch (cells outside the image are dropped at the flush)
            flags[k] = IN_PATCH;
            base[k] = (int)ly * PP + (int)lx;
        } else {
            flags[k] = taps_inside(s, p.W, p.H);
            base[k] = (int)((long)s.y0 * p.W + s.x0);   // >= -W - 1 > -2^31; read only together with a tap inside the image
        }
    }

    for (int i = tid; i < CG * PH * PP; i += NT) (&patch[0][0])[i] = 0.0;
    __syncthreads();

    for (long c0 = c_first; c0 < c_end; c0 += CG) {
        const int ncg = (int)min((long)CG, c_end - c0);
#pragma unroll
        for (int j = 0; j < CG; ++j) {
            if (j >= ncg) break;
            const long plane = (long)b * p.C + c0 + j;
            float v[PPT];   // the channel's values of the thread, requested together
#pragma unroll
            for (int k = 0; k < PPT; ++k) v[k] = pix[k] >= 0 ? in[plane * HW + pix[k]] : 0.f;
            float *O = out + plane * HW;
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int f = flags[k];
                if (f & IN_PATCH) {
                    double *cell = &patch[j][base[k]];
                    lds_add(cell, w[k][0] * v[k]);
                    lds_add(cell + 1, w[k][1] * v[k]);
                    lds_add(cell + PP, w[k][2] * v[k]);
                    lds_add(cell + PP + 1, w[k][3] * v[k]);
                } else if (f) {
                    float *g = O + (long)base[k];
                    if (f & A00) unsafeAtomicAdd(g, w[k][0] * v[k]);
                    if (f & A01) unsafeAtomicAdd(g + 1, w[k][1] * v[k]);
                    if (f & A10) unsafeAtomicAdd(g + p.W, w[k][2] * v[k]);
                    if (f & A11) unsafeAtomicAdd(g + p.W + 1, w[k][3] * v[k]);
                }
            }
        }
        __syncthreads();
        // flush: consecutive lanes take consecutive cells of a patch row; cells that are exactly zero (never touched) are skipped,
        // the others are added once and cleared for the next channel group
        for (int j = 0; j < ncg; ++j) {
            float *O = out + ((long)b * p.C + c0 + j) * HW;
            for (int i = tid; i < PH * PW; i += NT) {
                const int ly = i / PW, lx = i - ly * PW;
                const double v = patch[j][ly * PP + lx];
                if (v != 0.0) {
                    patch[j][ly * PP + lx] = 0.0;
                    const long gx = px0 + lx, gy = py0 + ly;
                    if (gx >= 0 && gx < p.W && gy >= 0 && gy < p.H) unsafeAtomicAdd(O + gy * p.W + gx, (float)v);
                }
            }
        }
        __syncthreads();
    }
}

// max |input| per plane as the bits of |input|: one integer atomicMax per workgroup and work item, whatever order they arrive in.
// A work item is MAX_PER x 256 consecutive values of one plane.
constexpr int MAX_PER = 16;
__global__ __launch_bounds__(NT) void splat_plane_max(const float *__restrict__ in, unsigned *__restrict__ pmax, long HW, long cpp, long items)
{
    __shared__ unsigned wmax[NT / FN2_WAVE];
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long plane = it / cpp, i0 = (it % cpp) * (long)(NT * MAX_PER) + threadIdx.x;
        float v[MAX_PER];
#pragma unroll
        for (int j = 0; j < MAX_PER; ++j) v[j] = i0 + (long)NT * j < HW ? in[plane * HW + i0 + (long)NT * j] : 0.f;
        unsigned m = 0u;
#pragma unroll
        for (int j = 0; j < MAX_PER; ++j) m = max(m, __float_as_uint(v[j]) & 0x7fffffffu);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
        if ((threadIdx.x & (FN2_WAVE - 1)) == 0) wmax[threadIdx.x / FN2_WAVE] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
            if (m != 0u) atomicMax(pmax + plane, m);
        }
        __syncthreads();
    }
}

// every cell of out is written: the converted sum, +0 for an all-zero plane, NaN for a plane with an inf or a NaN
__global__ __launch_bounds__(NT) void splat_convert(const unsigned long long *__restrict__ acc, const unsigned *__restrict__ pmax,
                                                    float *__restrict__ out, long HW, long ncell, int K)
{
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < ncell; i += (long)gridDim.x * NT) {
        int s = 0;
        const int kind = splat_scale(pmax[i / HW], K, s);
        out[i] = kind == SPLAT_PLANE_FINITE ? splat_unq(acc[i], s) : kind == SPLAT_PLANE_ZERO ? 0.f : __uint_as_float(0x7fc00000u);
    }
}

// one lane per source pixel; the four grad_out taps (+0 outside the image), grad_input written per channel, grad_flow summed in
// registers over ascending c.  An invalid pixel has taps of weight 0 and writes zeros.
template <bool GI, bool GF>
__global__ __launch_bounds__(NT) void splat_bwd(const float *__restrict__ in, const float *__restrict__ flow, const float *__restrict__ go,
                                                float *__restrict__ gin, float *__restrict__ gflow, const SplatP p)
{
    const Pixel q = pixel(p);
    if (!q.live) return;
    const long HW = (long)p.H * p.W;
    const float *fl = flow + (long)q.b * 2 * HW;
    const SplatTaps t = splat_taps(splat_pos(q.x, fl[q.pix]), splat_pos(q.y, fl[HW + q.pix]), p.W, p.H);
    const bool x0 = t.valid && t.x0 >= 0, x1 = t.valid && t.x0 + 1 < p.W, y0 = t.valid && t.y0 >= 0, y1 = t.valid && t.y0 + 1 < p.H;
    const long base = (long)t.y0 * p.W + t.x0;
    float gx = 0.f, gy = 0.f;
    for (int c = 0; c < p.C; ++c) {
        const long plane = (long)q.b * p.C + c;
        const float *G = go + plane * HW;
        const float g00 = y0 && x0 ? G[base] : 0.f, g01 = y0 && x1 ? G[base + 1] : 0.f;
        const float g10 = y1 && x0 ? G[base + p.W] : 0.f, g11 = y1 && x1 ? G[base + p.W + 1] : 0.f;
        if constexpr (GI) {
            float a = 0.f;
            a = a + t.w00 * g00;
            a = a + t.w01 * g01;
            a = a + t.w10 * g10;
            a = a + t.w11 * g11;
            gin[plane * HW + q.pix] = a;
        }
        if constexpr (GF) {
            const float v = in[plane * HW + q.pix];
            gx = gx + v * (t.by * (g01 - g00) + t.ay * (g11 - g10));
            gy = gy + v * (t.bx * (g10 - g00) + t.ax * (g11 - g01));
        }
    }
    if constexpr (GF) {
        float *gf = gflow + (long)q.b * 2 * HW;
        gf[q.pix] = gx;
        gf[HW + q.pix] = gy;
    }
}

constexpr unsigned SPLAT_WGS = 2048;   // eight workgroups of 256 threads per CU

unsigned capped(unsigned long long want) { return (unsigned)(want < (1ull << 20) ? want : (1ull << 20)); }

} // namespace

int splat_make_params(SplatP &p, int B, int C, int H, int W)
{
    if (B < 0 || C < 1 || H < 1 || W < 1) return FN2_EINVAL;
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= (1ull << 31)) return FN2_EUNSUPPORTED;
    const unsigned long long planes = (unsigned long long)B * (unsigned long long)C;
    if (planes >= (1ull << 31) || planes * hw >= (1ull << 48)) return FN2_EUNSUPPORTED;
    const unsigned long long chunks = (hw + NT - 1) / NT;
    const unsigned long long tx = ((unsigned long long)W + TW - 1) / TW, ty = ((unsigned long long)H + TH - 1) / TH;
    if ((unsigned long long)B * chunks >= (1ull << 31) || (unsigned long long)B * tx * ty >= (1ull << 31)) return FN2_EUNSUPPORTED;
    int K = 0;
    while ((1ull << K) < hw) ++K;
    // the tiled forward: a workgroup takes a tile and a run of channel groups, the runs sized for about SPLAT_WGS workgroups
    const unsigned long long tiles = (unsigned long long)B * tx * ty, groups = ((unsigned long long)C + CG - 1) / CG;
    unsigned long long per = groups * tiles / SPLAT_WGS;
    per = per < 1 ? 1 : per > groups ? groups : per;
    p = SplatP{B, C, H, W, (int)chunks, (int)tx, (int)ty, K, (int)per, (int)((groups + per - 1) / per)};
    return FN2_OK;
}

size_t splat_det_workspace_bytes(const SplatP &p)
{
    const size_t planes = (size_t)p.B * p.C;
    return (4 * planes + 255) / 256 * 256 + 8 * planes * (size_t)p.H * p.W;
}

int splat_forward(const float *in, const float *flow, float *out, const SplatP &p, bool tiled, hipStream_t s)
{
    const size_t bytes = sizeof(float) * (size_t)p.B * p.C * p.H * p.W;
    int rc = zero_fill_async(out, bytes, s);
    if (rc != FN2_OK) return rc;
    if (tiled)
        hipLaunchKernelGGL(splat_fwd_tiled, dim3((unsigned)p.B * p.tiles_x * p.tiles_y * p.group_runs), dim3(NT), 0, s, in, flow, out, p);
    else
        hipLaunchKernelGGL(splat_fwd_general<false>, dim3((unsigned)p.B * p.chunks), dim3(NT), 0, s, in, flow, out,
                           (unsigned long long *)nullptr, (const unsigned *)nullptr, p);
    return launch_status();
}

int splat_forward_det(const float *in, const float *flow, float *out, void *workspace, const SplatP &p, hipStream_t s)
{
    const long planes = (long)p.B * p.C, HW = (long)p.H * p.W;
    int rc = zero_fill_async(workspace, splat_det_workspace_bytes(p), s);
    if (rc != FN2_OK) return rc;
    unsigned *pmax = static_cast<unsigned *>(workspace);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + (4 * planes + 255) / 256 * 256);
    const long cpp = (HW + NT * MAX_PER - 1) / (NT * MAX_PER);
    hipLaunchKernelGGL(splat_plane_max, dim3(capped((unsigned long long)planes * cpp)), dim3(NT), 0, s, in, pmax, HW, cpp, planes * cpp);
    if ((rc = launch_status()) != FN2_OK) return rc;
    hipLaunchKernelGGL(splat_fwd_general<true>, dim3((unsigned)p.B * p.chunks), dim3(NT), 0, s, in, flow, (float *)nullptr, acc, pmax, p);
    if ((rc = launch_status()) != FN2_OK) return rc;
    hipLaunchKernelGGL(splat_convert, dim3(capped(((unsigned long long)planes * HW + NT - 1) / NT)), dim3(NT), 0, s, acc, pmax, out, HW,
                       planes * HW, p.K);
    return launch_status();
}

int splat_backward(const float *in, const float *flow, const float *go, float *gin, float *gflow, const SplatP &p, hipStream_t s)
{
    const dim3 grid((unsigned)p.B * p.chunks), block(NT);
    if (gin && gflow) hipLaunchKernelGGL((splat_bwd<true, true>), grid, block, 0, s, in, flow, go, gin, gflow, p);
    else if (gin) hipLaunchKernelGGL((splat_bwd<true, false>), grid, block, 0, s, in, flow, go, gin, gflow, p);
    else hipLaunchKernelGGL((splat_bwd<false, true>), grid, block, 0, s, in, flow, go, gin, gflow, p);
    return launch_status();
}

} // namespace fn2
