// correlation_1d.hip -- horizontal-search cost volume (Correlation1d: the stereo layer of DispNetC and its descendants) for gfx950.
//
//   out[b,o,y,x]      = (1/C) sum_c in1[b,c,y1,x1] * in2[b,c,y1,x1 + t*s2],   y1 = y*s1, x1 = x*s1 + md - pad, t = tmin + o
//   grad_in1[b,c,y,x] = (1/C) sum_t gO[b,o,y,x+pad-md]      * in2[b,c,y,x+t*s2]                       (s1 = 1)
//   grad_in2[b,c,y,x] = (1/C) sum_t gO[b,o,y,x-t*s2+pad-md] * in1[b,c,y,x-t*s2]
// t runs over -dr .. dr (single_direction 0), -dr .. 0 (-1) or 0 .. dr (+1), dr = md / s2; a term whose operand column or output
// column lies outside is absent, not a zero factor.  Padding is horizontal only; there is no kernel_size (it is 1).
//
// The arithmetic is the general 2-D kernel's (correlation_direct.hip) for k = 1, literally (corr_arith.h holds the channel sum both
// call), so that for pad == md the result is the centre row of the 2-D layer's displacement window bit for bit:
//   forward : four partial sums over the channels c = 0,1,2,3 (mod 4) in ascending order, the C % 4 leftover channels appended
//             to the first; 0 + ((s0 + s1) + (s2 + s3)); / C; one rounding to T; one product = fwd_prod<T> (corr_arith.h)
//   backward: one sequential sum over ascending t of (0 + gO) * v, starting at +0; / C; one rounding
//   accumulators: fp32 (float, half, bf16); double tensors: double in the backward, float in the forward (Acc<T>, as corr_*_direct)
// mul and add stay two roundings (-ffp-contract=off).
//
// General kernels (corr1d_*_general): one lane per output element / input element, any parameters, all four types.
//
// Tiled kernels (corr1d_*_tiled): s1 = s2 = 1, pad == md, 1 <= nOut <= 81, float / half / bf16; every element has the general
// kernel's bits (NaN where it has NaN).  The tiling is correlation_dense.hip's with the row displacement removed, and what the
// two have in common is one piece of code, corr_tiled.h: the four channels of one pixel side by side in LDS, the next four channels
// in flight from global memory (two buffers, one barrier per step), the forward's step, the backward's product loop.
//   forward : tile 32 x 4 pixels; one wave per group of nine displacements (NG waves, NG in {1,2,3,5,7,9}: the smallest that
//             covers nOut; displacements from nOut on are computed on zeros and not stored); one lane = 2 adjacent pixels x 9
//             displacements x 4 chains.  The in2 image is 4 rows of 32 + 9 NG - 1 columns that start at column tx0 + tmin: the
//             halo is horizontal only.  Odd LDS pitches (33, (31 + 9 NG) | 1 vectors), as in the dense kernel.
//   backward: tile 32 x 8 pixels, one lane per pixel; its nOut gO factors stay in registers (NB in {9,27,45,81} slots, the ones
//             from nOut on skipped by wave-uniform branches) while the channels stream past.  gradInput1 and gradInput2 are
//             separate workgroups (blockIdx.z parity) that differ in the sign of the displacement: for gradInput2 the rows are
//             staged mirrored, so both walk the LDS image with the same compile-time offsets.  The channels are split over
//             blockIdx.y where the tiles alone do not fill the chip.
// Every global load comes from inside the tensor (the address is clamped, then zero is selected); a store goes only to
// elements of the call's outputs.
#include <type_traits>

#include "corr1d.h"
#include "corr_tiled.h"

namespace fn2 {

// ---------------------------------------------------------------- shape math
int corr1d_output_shape(int H, int W, int pad, int md, int s1, int s2, int sd, int *nOut, int *oH, int *oW)
{
    if (H < 1 || W < 1 || pad < 0 || md < 0 || s1 < 1 || s2 < 1 || sd < -1 || sd > 1) return FN2_EINVAL;
    const long span = (long)W + 2L * pad - 2L * md;
    if (span < 1) return FN2_EINVAL;   // empty output
    const int dr = md / s2;
    if (nOut) *nOut = sd == 0 ? 2 * dr + 1 : dr + 1;
    if (oH) *oH = (H + s1 - 1) / s1;
    if (oW) *oW = (int)((span + s1 - 1) / s1);
    return FN2_OK;
}

int corr1d_make_params(Corr1dP &p, int B, int C, int H, int W, int pad, int md, int s1, int s2, int sd)
{
    if (B < 0 || C < 1) return FN2_EINVAL;
    const int rc = corr1d_output_shape(H, W, pad, md, s1, s2, sd, &p.nOut, &p.oH, &p.oW);
    if (rc != FN2_OK) return rc;
    p.B = B; p.C = C; p.H = H; p.W = W;
    p.pad = pad; p.md = md; p.s1 = s1; p.s2 = s2; p.sd = sd;
    p.dr = md / s2;
    p.tmin = sd == 1 ? 0 : -p.dr;
    return FN2_OK;
}

namespace {

// ================================================================ general kernels
template <typename T>
__global__ __launch_bounds__(256) void corr1d_fwd_general(const T *__restrict__ in1, const T *__restrict__ in2, T *__restrict__ out,
                                                          Corr1dP p, long total)
{
    const long HW = (long)p.H * p.W;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int bx = (int)(idx % p.oW);
        long r = idx / p.oW;
        const int by = (int)(r % p.oH);
        r /= p.oH;
        const int o = (int)(r % p.nOut);
        const int n = (int)(r / p.nOut);
        const int y1 = by * p.s1, x1 = bx * p.s1 + p.md - p.pad;
        const int x2 = x1 + (p.tmin + o) * p.s2;
        float acc = 0.0f;
        if (x1 >= 0 && x1 < p.W && x2 >= 0 && x2 < p.W) {   // otherwise the term is absent
            const T *pa = in1 + (long)n * p.C * HW + (long)y1 * p.W + x1;
            const T *pb = in2 + (long)n * p.C * HW + (long)y1 * p.W + x2;
            acc += fwd_channel_sum<T>(pa, pb, p.C, HW);   // four chains over the channels (corr_arith.h)
        }
        const int nelems = p.C;
        const float res = acc / nelems;
        out[idx] = (T)res;
    }
}

// One lane per (n, c, y, x) input element; both gradients.  stride1 = 1: oH = H, output column of image column x is x + pad - md.
template <typename T>
__global__ __launch_bounds__(256) void corr1d_bwd_general(const T *__restrict__ in1, const T *__restrict__ in2,
                                                          const T *__restrict__ gout, T *__restrict__ g1, T *__restrict__ g2,
                                                          Corr1dP p, long total)
{
    typedef typename Acc<T>::type A;
    const long HW = (long)p.H * p.W, oHW = (long)p.oH * p.oW;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % p.W);
        long r = idx / p.W;
        const int y = (int)(r % p.H);
        r /= p.H;
        const int c = (int)(r % p.C);
        const int n = (int)(r / p.C);
        const T *go = gout + (long)n * p.nOut * oHW + (long)y * p.oW;
        const T *a = in1 + ((long)n * p.C + c) * HW + (long)y * p.W;
        const T *b = in2 + ((long)n * p.C + c) * HW + (long)y * p.W;
        A sum1 = 0;
        const int ox1 = x + p.pad - p.md;
        if (ox1 >= 0 && ox1 < p.oW) {
            for (int o = 0; o < p.nOut; ++o) {
                const int xx = x + (p.tmin + o) * p.s2;
                if (xx < 0 || xx >= p.W) continue;
                A w = 0;
                w += (A)go[(long)o * oHW + ox1];
                sum1 += w * (A)b[xx];
            }
        }
        A sum2 = 0;
        for (int o = 0; o < p.nOut; ++o) {
            const int xx = x - (p.tmin + o) * p.s2;
            const int ox = xx + p.pad - p.md;
            if (ox < 0 || ox >= p.oW || xx < 0 || xx >= p.W) continue;
            A w = 0;
            w += (A)go[(long)o * oHW + ox];
            sum2 += w * (A)a[xx];
        }
        const A nelems = (A)p.C;
        g1[idx] = (T)(sum1 / nelems);
        g2[idx] = (T)(sum2 / nelems);
    }
}

template <typename T>
int fwd_general_launch(const void *in1, const void *in2, void *out, const Corr1dP &p, hipStream_t s)
{
    const long total = (long)p.B * p.nOut * p.oH * p.oW;
    if (total == 0) return FN2_OK;
    hipLaunchKernelGGL(corr1d_fwd_general<T>, dim3(stream_grid(total, 256L * 64)), dim3(256), 0, s, static_cast<const T *>(in1),
                       static_cast<const T *>(in2), static_cast<T *>(out), p, total);
    return launch_status();
}

template <typename T>
int bwd_general_launch(const void *in1, const void *in2, const void *gout, void *g1, void *g2, const Corr1dP &p, hipStream_t s)
{
    const long total = (long)p.B * p.C * p.H * p.W;
    if (total == 0) return FN2_OK;
    hipLaunchKernelGGL(corr1d_bwd_general<T>, dim3(stream_grid(total, 256L * 64)), dim3(256), 0, s, static_cast<const T *>(in1),
                       static_cast<const T *>(in2), static_cast<const T *>(gout), static_cast<T *>(g1), static_cast<T *>(g2), p, total);
    return launch_status();
}

// ================================================================ tiled kernels
constexpr int TILED_MAX_NOUT = 81;
constexpr int GD = 9;              // forward: displacements per wave
// waves per SIMD the backward is built for: 81 gO factors alone are 82 registers
constexpr int bwd_waves(int nb) { return nb > 45 ? 3 : 4; }

// ---------------------------------------------------------------- forward
template <typename T, int NG>
__global__ __launch_bounds__(NG * 64) void corr1d_fwd_tiled(const T *__restrict__ in1, const T *__restrict__ in2, T *__restrict__ out,
                                                            Corr1dP p, int tilesX, int vec)
{
    typedef typename Lds<T>::type L;
    typedef L l4 __attribute__((ext_vector_type(4)));
    constexpr int NT = NG * 64;
    constexpr int C2 = FTW + GD * NG - 1, P2 = C2 | 1, P1 = FTW + 1;
    constexpr int N1 = FTH * FTW, NPOS = N1 + FTH * C2;   // staged pixels per channel quad: the in1 tile, the in2 tile + halo
    constexpr int SA = FTH * P1, SZ = SA + FTH * P2;
    constexpr int NLD = (NPOS + NT - 1) / NT;
    __shared__ l4 sm[2][SZ];

    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;   // one wave per nine displacements
    const int xg = lane & 15, r = lane >> 4;
    const int tx0 = ((int)blockIdx.x % tilesX) * FTW, ty0 = ((int)blockIdx.x / tilesX) * FTH;
    const int n = blockIdx.z;
    const int HW = p.H * p.W;
    const T *a = in1 + (long)n * p.C * HW;
    const T *b = in2 + (long)n * p.C * HW;
    const int need = FTW + p.nOut - 1;   // in2 columns of the image that a stored displacement reads

    // what this lane stages of every quad: pixel e of the in1 tile or (e - N1) of the in2 tile; -1 = zero (outside the image)
    QuadStage<T, L, NLD, NT> st;
    st.C = p.C; st.HW = HW;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + i * NT;
        int row, col, x;
        bool ok = e < NPOS;
        if (e < N1) {
            row = e / FTW; col = e % FTW;
            x = tx0 + col;
            st.src[i] = a; st.lidx[i] = row * P1 + col;
        } else {
            const int e2 = e - N1;
            row = e2 / C2; col = e2 % C2;
            x = tx0 + p.tmin + col;
            st.src[i] = b; st.lidx[i] = SA + row * P2 + col;
            ok = ok && col < need;
        }
        const int y = ty0 + row;
        ok = ok && y < p.H && x >= 0 && x < p.W;
        st.goff[i] = ok ? y * p.W + x : -1;
        if (e >= NPOS) st.lidx[i] = -1;
    }

    f4 acc[2][GD];   // component = chain (channel mod 4)
#pragma unroll
    for (int px = 0; px < 2; ++px)
#pragma unroll
        for (int d = 0; d < GD; ++d) acc[px][d] = (f4){0.0f, 0.0f, 0.0f, 0.0f};

    const int nq = (p.C + 3) / 4, full = p.C / 4, rem = p.C & 3;
    const int offA = r * P1 + 2 * xg, offB = SA + r * P2 + 2 * xg + GD * grp;
    st.load(0);
    for (int q = 0; q < nq; ++q) {
        l4 *buf = sm[q & 1];
        st.step(buf, q, nq);
        fwd_quad<L, GD>(acc, buf, offA, offB, q < full, rem);
    }

    const int y = ty0 + r, x0 = tx0 + 2 * xg;
    if (y >= p.H || x0 >= p.W) return;
    const int nelems = p.C;
    const long obs = (long)p.nOut * HW;
#pragma unroll
    for (int d = 0; d < GD; ++d) {
        const int o = GD * grp + d;
        if (o >= p.nOut) break;   // wave-uniform: a displacement the call does not have
        T res2[2];
#pragma unroll
        for (int px = 0; px < 2; ++px) {
            const int x2 = x0 + px + p.tmin + o;
            const float sum = fwd_lane_sum(acc[px][d], x2 >= 0 && x2 < p.W);
            const float res = sum / nelems;
            res2[px] = (T)res;
        }
        store_results<T>(out + (long)n * obs + ((long)o * p.H + y) * p.W + x0, res2, vec, x0 + 1 < p.W);
    }
}

// ---------------------------------------------------------------- backward
// which = 0: gradInput1[c,y,x] = sum_t gO[o,y,x] * in2[c,y,x+t];  1: gradInput2[c,y,x] = sum_t gO[o,y,x-t] * in1[c,y,x-t].
// Slot ci of a staged row holds image column tx0 + tmin + ci (which = 0) or tx0 + 31 - tmin - ci (which = 1, mirrored), so the
// lane of tile column xl finds the operand of displacement o at slot (which ? 31 - xl : xl) + o in both.
template <typename T, int NB>
__global__ __launch_bounds__(BTW *BTH) __attribute__((amdgpu_waves_per_eu(bwd_waves(NB), bwd_waves(NB))))
void corr1d_bwd_tiled(const T *__restrict__ in1, const T *__restrict__ in2, const T *__restrict__ gout, T *__restrict__ g1,
                      T *__restrict__ g2, Corr1dP p, int tilesX, int qper)
{
    constexpr int NT = BTW * BTH;
    constexpr int CC = BTW + NB - 1, NPOS = BTH * CC;
    constexpr int NLD = (NPOS + NT - 1) / NT;
    __shared__ f4 sm[2][NPOS];
    const int tx0 = ((int)blockIdx.x % tilesX) * BTW, ty0 = ((int)blockIdx.x / tilesX) * BTH;
    const int which = blockIdx.z & 1, n = blockIdx.z >> 1;
    const int nq = (p.C + 3) / 4;
    const int qbeg = blockIdx.y * qper, qend = min(nq, qbeg + qper);
    if (qbeg >= qend) return;   // the whole workgroup
    const int HW = p.H * p.W;
    const long ib = (long)n * p.C * HW;
    const T *go = gout + (long)n * p.nOut * HW;
    const T *inp = (which ? in1 : in2) + ib;
    T *g = (which ? g2 : g1) + ib;
    const int nOut = p.nOut;
    const int need = BTW + nOut - 1;

    const int tid = threadIdx.x, xl = tid % BTW, yl = tid / BTW;
    const int y = ty0 + yl, x = tx0 + xl;
    const bool inimg = y < p.H && x < p.W;

    QuadStage<T, float, NLD, NT> st;   // BTH rows of `inp`, columns as above
    st.C = p.C; st.HW = HW;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + i * NT;
        const int row = e / CC, ci = e % CC;
        const int yy = ty0 + row, xx = which ? tx0 + BTW - 1 - p.tmin - ci : tx0 + p.tmin + ci;
        const bool ok = e < NPOS && ci < need && yy < p.H && xx >= 0 && xx < p.W;
        st.src[i] = inp;
        st.goff[i] = ok ? yy * p.W + xx : -1;
        st.lidx[i] = e < NPOS ? e : -1;
    }
    st.load(qbeg);

    // the gO factors of this pixel, once for all channels; 0 where the term is absent
    const int sgn = which ? -1 : 1;
    f2 wp[(NB + 1) / 2];   // factor o is half o & 1 of pair o / 2 (bwd_quad)
#pragma unroll
    for (int o = 0; o < NB; ++o) {
        const int ox = x + sgn * (p.tmin + o);   // the other operand's column
        const int sx = which ? ox : x;           // gO's column
        const bool ok = inimg && o < nOut && ox >= 0 && ox < p.W;
        float v = 0.0f;
        v += (float)go[ok ? o * HW + y * p.W + sx : 0];
        wp[o / 2][o & 1] = ok ? v : 0.0f;
    }
    if (NB & 1) wp[NB / 2][1] = 0.0f;

    const float nelems = (float)p.C;
    const int centre = yl * CC + (which ? BTW - 1 - xl : xl);
    for (int q = qbeg; q < qend; ++q) {
        f4 *buf = sm[(q - qbeg) & 1];
        st.step(buf, q, qend);
        // a group of displacements from nOut on is skipped as a whole, a displacement from nOut on inside the last group by itself:
        // both wave-uniform
        const f4 sum = bwd_quad<NB>(buf + centre, wp, nOut, [](int t) { return t; });
        if (inimg) bwd_store_quad(g, y * p.W + x, q, p.C, HW, sum, nelems);
    }
}

template <typename T, int NG>
int fwd_tiled_launch(const void *in1, const void *in2, void *out, const Corr1dP &p, hipStream_t s)
{
    const int tilesX = (p.W + FTW - 1) / FTW, tilesY = (p.H + FTH - 1) / FTH;
    const int vec = fwd_pairs_aligned(p.W, (long)p.nOut * p.H * p.W, out, sizeof(T));
    hipLaunchKernelGGL((corr1d_fwd_tiled<T, NG>), dim3(tilesX * tilesY, 1, p.B), dim3(NG * 64), 0, s, static_cast<const T *>(in1),
                       static_cast<const T *>(in2), static_cast<T *>(out), p, tilesX, vec);
    return launch_status();
}

template <typename T, int NB>
int bwd_tiled_launch(const void *in1, const void *in2, const void *gout, void *g1, void *g2, const Corr1dP &p, hipStream_t s)
{
    const int tilesX = (p.W + BTW - 1) / BTW, tilesY = (p.H + BTH - 1) / BTH;
    const int nq = (p.C + 3) / 4;
    int split;
    const int qper = bwd_channel_split((long)tilesX * tilesY * p.B * 2, nq, &split);
    hipLaunchKernelGGL((corr1d_bwd_tiled<T, NB>), dim3(tilesX * tilesY, split, p.B * 2), dim3(BTW * BTH), 0, s,
                       static_cast<const T *>(in1), static_cast<const T *>(in2), static_cast<const T *>(gout), static_cast<T *>(g1),
                       static_cast<T *>(g2), p, tilesX, qper);
    return launch_status();
}

template <typename T>
int fwd_tiled_groups(const void *in1, const void *in2, void *out, const Corr1dP &p, hipStream_t s)
{
    const int ng = (p.nOut + GD - 1) / GD;
    if (ng <= 1) return fwd_tiled_launch<T, 1>(in1, in2, out, p, s);
    if (ng <= 2) return fwd_tiled_launch<T, 2>(in1, in2, out, p, s);
    if (ng <= 3) return fwd_tiled_launch<T, 3>(in1, in2, out, p, s);
    if (ng <= 5) return fwd_tiled_launch<T, 5>(in1, in2, out, p, s);
    if (ng <= 7) return fwd_tiled_launch<T, 7>(in1, in2, out, p, s);
    return fwd_tiled_launch<T, 9>(in1, in2, out, p, s);
}

template <typename T>
int bwd_tiled_slots(const void *in1, const void *in2, const void *gout, void *g1, void *g2, const Corr1dP &p, hipStream_t s)
{
    if (p.nOut <= 9) return bwd_tiled_launch<T, 9>(in1, in2, gout, g1, g2, p, s);
    if (p.nOut <= 27) return bwd_tiled_launch<T, 27>(in1, in2, gout, g1, g2, p, s);
    if (p.nOut <= 45) return bwd_tiled_launch<T, 45>(in1, in2, gout, g1, g2, p, s);
    return bwd_tiled_launch<T, 81>(in1, in2, gout, g1, g2, p, s);
}

} // namespace

int corr1d_forward_general(const void *in1, const void *in2, void *out, int dtype, const Corr1dP &p, hipStream_t s)
{
    switch (dtype) {
    case FN2_F32: return fwd_general_launch<float>(in1, in2, out, p, s);
    case FN2_F16: return fwd_general_launch<half_t>(in1, in2, out, p, s);
    case FN2_F64: return fwd_general_launch<double>(in1, in2, out, p, s);
    case FN2_BF16: return fwd_general_launch<bf16_t>(in1, in2, out, p, s);
    default: return FN2_EDTYPE;
    }
}

int corr1d_backward_general(const void *in1, const void *in2, const void *gout, void *g1, void *g2, int dtype, const Corr1dP &p,
                            hipStream_t s)
{
    switch (dtype) {
    case FN2_F32: return bwd_general_launch<float>(in1, in2, gout, g1, g2, p, s);
    case FN2_F16: return bwd_general_launch<half_t>(in1, in2, gout, g1, g2, p, s);
    case FN2_F64: return bwd_general_launch<double>(in1, in2, gout, g1, g2, p, s);
    case FN2_BF16: return bwd_general_launch<bf16_t>(in1, in2, gout, g1, g2, p, s);
    default: return FN2_EDTYPE;
    }
}

bool corr1d_tiled_applicable(int dtype, const Corr1dP &p)
{
    return (dtype == FN2_F32 || dtype == FN2_F16 || dtype == FN2_BF16) && p.C >= 1 && p.s1 == 1 && p.s2 == 1 && p.pad == p.md &&
           p.nOut >= 1 && p.nOut <= TILED_MAX_NOUT && tiled_fits(p);
}

// What AUTO asks before it takes the tiled FORWARD: all 81 displacements and at least 768 workgroups (batch x tiles of 32 x 4
// pixels).  A workgroup walks the channels of its tile in steps of four at about two microseconds per step, whatever the step
// holds: one global -> LDS -> barrier -> read round trip that nothing hides at one 9-wave workgroup per CU.  So its time follows
// the number of workgroups and C, not nOut, while the general kernel's follows the products it forms.  Measured on an MI355X at
// B = 8, md 40 (profiles/corr1d_micro.json), general / tiled: nOut 81 at 1152 workgroups (96 x 192) 1.4-2.5x
// float, 1.1-1.2x half, 1.2-1.3x bf16, at 768 (32 x 96 x 128) 1.4x float, 1.25x half; at 288 (48 x 96) 1.0 / 0.72 / 0.86x, at 96
// (24 x 48) 0.6-0.8x; one-sided search (nOut 41) at 1152 workgroups 0.65-0.9x.  768 is the smallest count measured to win and 81
// the only nOut: between the measured points nothing is claimed and the general kernel stays.  The backward splits the channels
// over workgroups and wins at every measured size (1.7-3.3x).
bool corr1d_forward_pays(const Corr1dP &p)
{
    const long tiles = (long)((p.W + FTW - 1) / FTW) * ((p.H + FTH - 1) / FTH);
    return p.nOut == TILED_MAX_NOUT && tiles * p.B >= 768;
}

int corr1d_forward_tiled(const void *in1, const void *in2, void *out, int dtype, const Corr1dP &p, hipStream_t s)
{
    if (!corr1d_tiled_applicable(dtype, p)) return FN2_EUNSUPPORTED;
    if (p.B == 0) return FN2_OK;
    switch (dtype) {
    case FN2_F32: return fwd_tiled_groups<float>(in1, in2, out, p, s);
    case FN2_F16: return fwd_tiled_groups<half_t>(in1, in2, out, p, s);
    case FN2_BF16: return fwd_tiled_groups<bf16_t>(in1, in2, out, p, s);
    default: return FN2_EUNSUPPORTED;
    }
}

int corr1d_backward_tiled(const void *in1, const void *in2, const void *gout, void *g1, void *g2, int dtype, const Corr1dP &p,
                          hipStream_t s)
{
    if (!corr1d_tiled_applicable(dtype, p)) return FN2_EUNSUPPORTED;
    if (p.B == 0) return FN2_OK;
    switch (dtype) {
    case FN2_F32: return bwd_tiled_slots<float>(in1, in2, gout, g1, g2, p, s);
    case FN2_F16: return bwd_tiled_slots<half_t>(in1, in2, gout, g1, g2, p, s);
    case FN2_BF16: return bwd_tiled_slots<bf16_t>(in1, in2, gout, g1, g2, p, s);
    default: return FN2_EUNSUPPORTED;
    }
}

} // namespace fn2
