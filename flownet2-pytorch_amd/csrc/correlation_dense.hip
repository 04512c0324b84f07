// correlation_dense.hip -- LDS-tiled correlation kernels for dense stride-1 cost volumes on gfx950: the configuration PWC-Net,
// IRR-PWC and LiteFlowNet call, Correlation(pad_size=md, kernel_size=1, max_displacement=md, stride1=1, stride2=1).
//
// Domain (corr_dense_applicable): kernel_size 1, stride1 1, stride2 1, pad_size == max_displacement == md, 1 <= md <= 4;
// float, half and bfloat16 tensors; any B, C >= 1, H, W, element-aligned pointers.  A shape beyond the 32-bit offsets of one
// batch item or the grid limits is declined (FN2_EUNSUPPORTED, nothing launched) and the dispatcher runs the general kernel.
//
// Contract: every output element has the bits of the general kernel (correlation_direct.hip, FN2_CORR_DIRECT) for the same call.
// The arithmetic is therefore that kernel's, restated for k = 1, s1 = 1:
//   forward : four partial sums over the channels c = 0,1,2,3 (mod 4) in ascending order, the C % 4 leftover channels appended
//             to the first; 0 + ((s0 + s1) + (s2 + s3)); / C; LeakyReLU; one product = fwd_prod<T> (corr_arith.h)
//   backward: one sequential fp32 sum over the displacement planes in ascending order of (0 + gO) * v; / C; rounded once to T
//   a term whose second operand lies outside the image is absent: the forward selects 0 instead of the sum (the sum may be NaN
//   from inf * 0 on the zero-filled halo); the backward zeroes the gO factor as well as the halo, and sum + (+0 * +0) is sum for
//   every sum a chain that starts at +0 can hold.
// mul and add stay two roundings (-ffp-contract=off); packed and scalar fp32 / f16 instructions round alike.
//
// Design.  The channel-quad tiling of corr_tiled.h (shared with correlation_1d.hip): the staging pipeline, the forward's step and
// lane sum, the backward's product loop and the launch arithmetic live there; here is what the 2-D search makes its own.
//   forward : tile 32 x 4 pixels, one wave per dy row (2md+1 waves), one lane = 2 adjacent pixels x (2md+1) dx x 4 chains
//             (72 accumulators at md = 4); per 4 channels a lane reads 2 + 2md+2 vectors for 8(2md+1) products.
//             LDS pitches are odd (33, 32+2md+1 vectors): the lanes of one row use the even 16-byte slots, those of the next row
//             the odd ones -- conflict-free for ds_read_b128's 16-lane groups and ds_read_b64's halves.
//   backward: tile 32 x 8 pixels, one lane = one pixel; its (2md+1)^2 gO factors stay in registers for all channels, every channel
//             quad is one ds_read_b128 per displacement (32 consecutive slots per half wave: conflict-free).  gradInput1 and
//             gradInput2 are separate workgroups (blockIdx.z parity) that differ in the sign of the displacement; the channels
//             are split over blockIdx.y where the tiles alone do not fill the chip.
#include <type_traits>

#include "corr_params.h"
#include "corr_tiled.h"

namespace fn2 {

namespace {

constexpr int DENSE_MAX_MD = 4;
// waves per SIMD the backward is built for: the (2md+1)^2 gO factors alone are 82 registers at md = 4
constexpr int bwd_waves(int md) { return md >= 4 ? 3 : 4; }

// ---------------------------------------------------------------- forward
template <typename T, int MD>
__global__ __launch_bounds__((2 * MD + 1) * 64) void corr_fwd_dense(const T *__restrict__ in1, const T *__restrict__ in2,
                                                                    T *__restrict__ out, CorrP p, int tilesX, int vec)
{
    typedef typename Lds<T>::type L;
    typedef L l4 __attribute__((ext_vector_type(4)));
    constexpr int D = 2 * MD + 1, NT = D * 64;
    constexpr int R2 = FTH + 2 * MD, C2 = FTW + 2 * MD, P2 = C2 + 1, P1 = FTW + 1;
    constexpr int N1 = FTH * FTW, NPOS = N1 + R2 * C2;   // staged pixels per channel quad: the in1 tile, the in2 tile + halo
    constexpr int SA = FTH * P1, SZ = SA + R2 * P2;
    constexpr int NLD = (NPOS + NT - 1) / NT;
    __shared__ l4 sm[2][SZ];

    const int tid = threadIdx.x, lane = tid & 63, dyI = tid >> 6;   // one wave per dy
    const int xg = lane & 15, r = lane >> 4;
    const int tx0 = ((int)blockIdx.x % tilesX) * FTW, ty0 = ((int)blockIdx.x / tilesX) * FTH;
    const int n = blockIdx.z;
    const int HW = p.H * p.W;
    const T *a = in1 + (long)n * p.C * HW;
    const T *b = in2 + (long)n * p.C * HW;

    // what this lane stages of every quad: pixel e of the in1 tile or (e - N1) of the in2 tile; -1 = outside the image (zero)
    QuadStage<T, L, NLD, NT> st;
    st.C = p.C; st.HW = HW;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + i * NT;
        int row, col, y, x;
        if (e < N1) {
            row = e / FTW; col = e % FTW;
            y = ty0 + row; x = tx0 + col;
            st.src[i] = a; st.lidx[i] = row * P1 + col;
        } else {
            const int e2 = e - N1;
            row = e2 / C2; col = e2 % C2;
            y = ty0 - MD + row; x = tx0 - MD + col;
            st.src[i] = b; st.lidx[i] = SA + row * P2 + col;
        }
        const bool ok = e < NPOS && y >= 0 && y < p.H && x >= 0 && x < p.W;
        st.goff[i] = ok ? y * p.W + x : -1;
        if (e >= NPOS) st.lidx[i] = -1;
    }

    f4 acc[2][D];   // component = chain (channel mod 4)
#pragma unroll
    for (int px = 0; px < 2; ++px)
#pragma unroll
        for (int dx = 0; dx < D; ++dx) acc[px][dx] = (f4){0.0f, 0.0f, 0.0f, 0.0f};

    const int nq = (p.C + 3) / 4, full = p.C / 4, rem = p.C & 3;
    const int offA = r * P1 + 2 * xg, offB = SA + (r + dyI) * P2 + 2 * xg;
    st.load(0);
    for (int q = 0; q < nq; ++q) {
        l4 *buf = sm[q & 1];
        st.step(buf, q, nq);
        fwd_quad<L, D>(acc, buf, offA, offB, q < full, rem);
    }

    const int y = ty0 + r, x0 = tx0 + 2 * xg;
    if (y >= p.H || x0 >= p.W) return;
    const int y2 = y + dyI - MD;
    const bool yok = y2 >= 0 && y2 < p.H;
    const int nelems = p.k * p.k * p.C;
    T *o = out + (long)n * p.out_bs + ((long)dyI * D * p.H + y) * p.W + x0;
#pragma unroll
    for (int dx = 0; dx < D; ++dx) {
        T res2[2];
#pragma unroll
        for (int px = 0; px < 2; ++px) {
            const int x2 = x0 + px + dx - MD;
            const float sum = fwd_lane_sum(acc[px][dx], yok && x2 >= 0 && x2 < p.W);
            float res = sum / nelems;
            if (p.slope != 1.0f) res = res > 0.0f ? res : (float)(T)res * p.slope;
            res2[px] = (T)res;
        }
        store_results<T>(o + (long)dx * HW, res2, vec, x0 + 1 < p.W);
    }
}

// ---------------------------------------------------------------- backward
// which = 0: gradInput1[c,y,x] = sum_tc gO[tc,y,x] * in2[c,y+dy,x+dx];  1: gradInput2[c,y,x] = sum_tc gO[tc,y-dy,x-dx] * in1[c,y-dy,x-dx].
// The two differ in the sign of the displacement.  For gradInput2 the tile is staged point-mirrored, so that both walk the LDS
// image with the same compile-time offsets (+dy, +dx from the lane's centre) and share one instruction stream.
template <typename T, int MD>
__global__ __launch_bounds__(BTW *BTH) __attribute__((amdgpu_waves_per_eu(bwd_waves(MD), bwd_waves(MD))))
void corr_bwd_dense(const T *__restrict__ in1, const T *__restrict__ in2, const T *__restrict__ gout, T *__restrict__ g1,
                    T *__restrict__ g2, CorrP p, int tilesX, int qper)
{
    constexpr int D = 2 * MD + 1, NT = BTW * BTH;
    constexpr int R = BTH + 2 * MD, CC = BTW + 2 * MD, NPOS = R * CC;
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

    const int tid = threadIdx.x, xl = tid % BTW, yl = tid / BTW;
    const int y = ty0 + yl, x = tx0 + xl;
    const bool inimg = y < p.H && x < p.W;

    QuadStage<T, float, NLD, NT> st;   // the tile + halo of `inp`; for gradInput2 written point-mirrored
    st.C = p.C; st.HW = HW;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + i * NT;
        const int row = e / CC, col = e % CC;
        const int yy = ty0 - MD + row, xx = tx0 - MD + col;
        const bool ok = e < NPOS && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
        st.src[i] = inp;
        st.goff[i] = ok ? yy * p.W + xx : -1;
        st.lidx[i] = e < NPOS ? (which ? NPOS - 1 - e : e) : -1;
    }
    st.load(qbeg);

    // the gO factors of this pixel, once for all channels; 0 where the term is absent
    const int sgn = which ? -1 : 1;
    f2 wp[(D * D + 1) / 2];   // factor tc is half tc & 1 of pair tc / 2 (bwd_quad)
#pragma unroll
    for (int tc = 0; tc < D * D; ++tc) {
        const int dy = tc / D - MD, dx = tc % D - MD;
        const int oy = y + sgn * dy, ox = x + sgn * dx;         // the other operand's pixel
        const int sy = which ? oy : y, sx = which ? ox : x;     // gO's pixel
        const bool ok = inimg && oy >= 0 && oy < p.H && ox >= 0 && ox < p.W;
        float v = 0.0f;
        v += (float)go[tc * HW + (ok ? sy * p.W + sx : 0)];
        wp[tc / 2][tc & 1] = ok ? v : 0.0f;
    }
    if (D * D & 1) wp[D * D / 2][1] = 0.0f;

    const float nelems = (float)(p.k * p.k * p.C);
    const int c0 = (yl + MD) * CC + xl + MD;
    const int centre = which ? NPOS - 1 - c0 : c0;
    for (int q = qbeg; q < qend; ++q) {
        f4 *buf = sm[(q - qbeg) & 1];
        st.step(buf, q, qend);
        const f4 sum = bwd_quad<D * D>(buf + centre, wp, D * D, [](int t) { return ((t / D) - MD) * CC + (t % D) - MD; });
        if (inimg) bwd_store_quad(g, y * p.W + x, q, p.C, HW, sum, nelems);
    }
}

template <typename T, int MD>
int fwd_dense_launch(const void *in1, const void *in2, void *out, const CorrP &p, hipStream_t s)
{
    const int tilesX = (p.W + FTW - 1) / FTW, tilesY = (p.H + FTH - 1) / FTH;
    const int vec = fwd_pairs_aligned(p.W, p.out_bs, out, sizeof(T));
    hipLaunchKernelGGL((corr_fwd_dense<T, MD>), dim3(tilesX * tilesY, 1, p.B), dim3((2 * MD + 1) * 64), 0, s,
                       static_cast<const T *>(in1), static_cast<const T *>(in2), static_cast<T *>(out), p, tilesX, vec);
    return launch_status();
}

template <typename T, int MD>
int bwd_dense_launch(const void *in1, const void *in2, const void *gout, void *g1, void *g2, const CorrP &p, hipStream_t s)
{
    const int tilesX = (p.W + BTW - 1) / BTW, tilesY = (p.H + BTH - 1) / BTH;
    const int nq = (p.C + 3) / 4;
    int split;
    const int qper = bwd_channel_split((long)tilesX * tilesY * p.B * 2, nq, &split);
    hipLaunchKernelGGL((corr_bwd_dense<T, MD>), dim3(tilesX * tilesY, split, p.B * 2), dim3(BTW * BTH), 0, s,
                       static_cast<const T *>(in1), static_cast<const T *>(in2), static_cast<const T *>(gout),
                       static_cast<T *>(g1), static_cast<T *>(g2), p, tilesX, qper);
    return launch_status();
}

template <typename T>
int fwd_dense_md(const void *in1, const void *in2, void *out, const CorrP &p, hipStream_t s)
{
    switch (p.md) {
    case 1: return fwd_dense_launch<T, 1>(in1, in2, out, p, s);
    case 2: return fwd_dense_launch<T, 2>(in1, in2, out, p, s);
    case 3: return fwd_dense_launch<T, 3>(in1, in2, out, p, s);
    case 4: return fwd_dense_launch<T, 4>(in1, in2, out, p, s);
    default: return FN2_EUNSUPPORTED;
    }
}

template <typename T>
int bwd_dense_md(const void *in1, const void *in2, const void *gout, void *g1, void *g2, const CorrP &p, hipStream_t s)
{
    switch (p.md) {
    case 1: return bwd_dense_launch<T, 1>(in1, in2, gout, g1, g2, p, s);
    case 2: return bwd_dense_launch<T, 2>(in1, in2, gout, g1, g2, p, s);
    case 3: return bwd_dense_launch<T, 3>(in1, in2, gout, g1, g2, p, s);
    case 4: return bwd_dense_launch<T, 4>(in1, in2, gout, g1, g2, p, s);
    default: return FN2_EUNSUPPORTED;
    }
}

} // namespace

bool corr_dense_applicable(int dtype, const CorrP &p)
{
    return (dtype == FN2_F32 || dtype == FN2_F16 || dtype == FN2_BF16) && p.C >= 1 && p.k == 1 && p.s1 == 1 && p.s2 == 1 && p.pad == p.md &&
           p.md >= 1 && p.md <= DENSE_MAX_MD;
}

// What FN2_CORR_AUTO asks before it takes the dense FORWARD: at least 192 workgroups (batch x 32 x 4-pixel tiles).  A workgroup
// walks all channels of its tile in steps of four, about a microsecond per step whatever the tile holds, so a small map leaves
// most CUs idle behind a few long serial walks, where the general kernel spreads the same products over every lane of the chip.
// Measured on an MI355X at B = 8: 192 workgroups (64 x 48 x 64) 1.5-1.7x faster than the general kernel, 48
// (96 x 24 x 32) 0.6-0.75x, 16 (196 x 6 x 8) 0.2-0.3x.  The backward splits the channels over workgroups and wins at every level.
// C is deliberately no part of the predicate: a workgroup's serial walk is C / 4 steps and the general kernel's time is
// proportional to C as well, so their ratio is set by how many workgroups there are, not by how long each one runs.
bool corr_dense_forward_pays(const CorrP &p)
{
    const long tiles = (long)((p.W + FTW - 1) / FTW) * ((p.H + FTH - 1) / FTH);
    return tiles * p.B >= 192;
}

int corr_forward_dense(const CorrCall &c, hipStream_t s)
{
    if (!corr_dense_applicable(c.dtype, c.p) || !tiled_fits(c.p)) return FN2_EUNSUPPORTED;
    if (c.p.B == 0) return FN2_OK;
    switch (c.dtype) {
    case FN2_F32: return fwd_dense_md<float>(c.in1, c.in2, c.out, c.p, s);
    case FN2_F16: return fwd_dense_md<half_t>(c.in1, c.in2, c.out, c.p, s);
    case FN2_BF16: return fwd_dense_md<bf16_t>(c.in1, c.in2, c.out, c.p, s);
    default: return FN2_EUNSUPPORTED;
    }
}

int corr_backward_dense(const CorrCall &c, hipStream_t s)
{
    if (!corr_dense_applicable(c.dtype, c.p) || !tiled_fits(c.p)) return FN2_EUNSUPPORTED;
    if (c.p.B == 0) return FN2_OK;
    switch (c.dtype) {
    case FN2_F32: return bwd_dense_md<float>(c.in1, c.in2, c.gout, c.g1, c.g2, c.p, s);
    case FN2_F16: return bwd_dense_md<half_t>(c.in1, c.in2, c.gout, c.g1, c.g2, c.p, s);
    case FN2_BF16: return bwd_dense_md<bf16_t>(c.in1, c.in2, c.gout, c.g1, c.g2, c.p, s);
    default: return FN2_EUNSUPPORTED;
    }
}

} // namespace fn2
