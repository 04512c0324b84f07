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
// Design.  A workgroup owns one batch item and a tile of pixels and walks the channels four at a time.  The four channels of one
// pixel are staged side by side (16 bytes for fp32 / bf16-as-fp32, 8 bytes for half), so every LDS read is one aligned
// ds_read_b128 / b64 whatever the displacement, and the four lanes of the vector are the forward's four chains.  The next four
// channels travel from global memory into registers while the current ones are multiplied (two LDS buffers, one barrier per
// step).
//   forward : tile 32 x 4 pixels, one wave per dy row (2md+1 waves), one lane = 2 adjacent pixels x (2md+1) dx x 4 chains
//             (72 accumulators at md = 4); per 4 channels a lane reads 2 + 2md+2 vectors for 8(2md+1) products.
//             LDS pitches are odd (33, 32+2md+1 vectors): the lanes of one row use the even 16-byte slots, those of the next row
//             the odd ones -- conflict-free for ds_read_b128's 16-lane groups and ds_read_b64's halves.
//   backward: tile 32 x 8 pixels, one lane = one pixel; its (2md+1)^2 gO factors stay in registers for all channels, every channel
//             quad is one ds_read_b128 per displacement (32 consecutive slots per half wave: conflict-free).  gradInput1 and
//             gradInput2 are separate workgroups (blockIdx.z parity) that differ in the sign of the displacement; the channels
//             are split over blockIdx.y where the tiles alone do not fill the chip.
#include <type_traits>

#include "corr_arith.h"
#include "corr_params.h"

namespace fn2 {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int DENSE_MAX_MD = 4;
constexpr int FTW = 32, FTH = 4;   // forward tile (pixels)
constexpr int BTW = 32, BTH = 8;   // backward tile
constexpr int BG = 3;              // backward: displacements per scheduling group
// waves per SIMD the backward is built for: the (2md+1)^2 gO factors alone are 82 registers at md = 4
constexpr int bwd_waves(int md) { return md >= 4 ? 3 : 4; }

// element type of the forward's LDS image: bf16 is widened (its products are formed in fp32), half is multiplied in half
template <typename T> struct Lds { typedef float type; };
template <> struct Lds<half_t> { typedef half_t type; };

template <typename T> __device__ __forceinline__ void store_pair(T *p, T v0, T v1)
{
    if constexpr (sizeof(T) == 4) {
        store_out(reinterpret_cast<f2 *>(p), (f2){v0, v1});
    } else {
        typedef T t2 __attribute__((ext_vector_type(2)));
        store_out(reinterpret_cast<unsigned *>(p), __builtin_bit_cast(unsigned, (t2){v0, v1}));
    }
}

// (w[hi], w[hi]) * v as one packed multiply: op_sel picks the half of the pair `w` for both results, so a broadcast factor costs
// no register pair of its own (the compiler's own v_pk_mul_f32 keeps (w, w) for every displacement and spills).  Two roundings
// per mul + add as everywhere: the add is a separate instruction.
__device__ __forceinline__ f2 pk_mul_bcast(bool hi, f2 w, f2 v)   // hi: a constant once the caller's loop is unrolled
{
    f2 r;
    if (hi) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(w), "v"(v));
    else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(r) : "v"(w), "v"(v));
    return r;
}

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
    const T *src[NLD];
    int goff[NLD], lidx[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + i * NT;
        int row, col, y, x;
        if (e < N1) {
            row = e / FTW; col = e % FTW;
            y = ty0 + row; x = tx0 + col;
            src[i] = a; lidx[i] = row * P1 + col;
        } else {
            const int e2 = e - N1;
            row = e2 / C2; col = e2 % C2;
            y = ty0 - MD + row; x = tx0 - MD + col;
            src[i] = b; lidx[i] = SA + row * P2 + col;
        }
        const bool ok = e < NPOS && y >= 0 && y < p.H && x >= 0 && x < p.W;
        goff[i] = ok ? y * p.W + x : -1;
        if (e >= NPOS) lidx[i] = -1;
    }

    l4 val[NLD];
    auto gload = [&](int q) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 4 * q + k;   // always a load from inside the tensor (no branch around it), then the select
                const L v = (L)src[i][max(goff[i], 0) + min(c, p.C - 1) * HW];
                val[i][k] = (goff[i] >= 0 && c < p.C) ? v : (L)0.0f;
            }
        }
    };

    f4 acc[2][D];   // component = chain (channel mod 4)
#pragma unroll
    for (int px = 0; px < 2; ++px)
#pragma unroll
        for (int dx = 0; dx < D; ++dx) acc[px][dx] = (f4){0.0f, 0.0f, 0.0f, 0.0f};

    const int nq = (p.C + 3) / 4, full = p.C / 4, rem = p.C & 3;
    const int offA = r * P1 + 2 * xg, offB = SA + (r + dyI) * P2 + 2 * xg;
    gload(0);
    for (int q = 0; q < nq; ++q) {
        l4 *buf = sm[q & 1];
#pragma unroll
        for (int i = 0; i < NLD; ++i)
            if (lidx[i] >= 0) buf[lidx[i]] = val[i];
        __syncthreads();   // the only barrier of a step: the buffer written next was last read before this one
        if (q + 1 < nq) gload(q + 1);
        const l4 a0 = buf[offA], a1 = buf[offA + 1];
        l4 bv[D + 1];
#pragma unroll
        for (int j = 0; j < D + 1; ++j) bv[j] = buf[offB + j];
        if (q < full) {
#pragma unroll
            for (int dx = 0; dx < D; ++dx) {
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    const l4 av = px ? a1 : a0;
                    const l4 w = bv[dx + px];
                    f4 pr;
#pragma unroll
                    for (int k = 0; k < 4; ++k) pr[k] = fwd_prod<L>(av[k], w[k]);
                    acc[px][dx] += pr;
                }
            }
        } else {   // the C % 4 leftover channels go to the first chain, in order
#pragma unroll
            for (int dx = 0; dx < D; ++dx) {
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    const l4 av = px ? a1 : a0;
                    const l4 w = bv[dx + px];
                    float s0 = acc[px][dx][0];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (k < rem) s0 += fwd_prod<L>(av[k], w[k]);
                    acc[px][dx][0] = s0;
                }
            }
        }
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
            const f4 s = acc[px][dx];
            float sum = 0.0f;
            sum += (s[0] + s[1]) + (s[2] + s[3]);
            const int x2 = x0 + px + dx - MD;
            if (!(yok && x2 >= 0 && x2 < p.W)) sum = 0.0f;   // absent, not zero-multiplied
            float res = sum / nelems;
            if (p.slope != 1.0f) res = res > 0.0f ? res : (float)(T)res * p.slope;
            res2[px] = (T)res;
        }
        T *od = o + (long)dx * HW;
        if (vec) {
            store_pair<T>(od, res2[0], res2[1]);
        } else {
            store_out(od, res2[0]);
            if (x0 + 1 < p.W) store_out(od + 1, res2[1]);
        }
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

    int goff[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + i * NT;
        const int row = e / CC, col = e % CC;
        const int yy = ty0 - MD + row, xx = tx0 - MD + col;
        const bool ok = e < NPOS && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
        goff[i] = ok ? yy * p.W + xx : -1;
    }
    f4 val[NLD];
    auto gload = [&](int q) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 4 * q + k;   // always a load from inside the tensor (no branch around it), then the select
                const float v = (float)inp[max(goff[i], 0) + min(c, p.C - 1) * HW];
                val[i][k] = (goff[i] >= 0 && c < p.C) ? v : 0.0f;
            }
        }
    };
    gload(qbeg);

    // the gO factors of this pixel, once for all channels; 0 where the term is absent
    const int sgn = which ? -1 : 1;
    f2 wp[(D * D + 1) / 2];   // factor tc is half tc & 1 of pair tc / 2
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
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + i * NT;
            if (e < NPOS) buf[which ? NPOS - 1 - e : e] = val[i];
        }
        __syncthreads();   // the only barrier of a step: the buffer written next was last read before this one
        if (q + 1 < qend) gload(q + 1);
        const f4 *ctr = buf + centre;
        f2 s01 = (f2){0.0f, 0.0f}, s23 = (f2){0.0f, 0.0f};
        // BG displacements at a time, the reads of the next group in flight: left alone, the scheduler forms every product first
        // (they are independent, the two sums are chains) and spills them
        f4 cur[BG], nxt[BG];
#pragma unroll
        for (int i = 0; i < BG; ++i) cur[i] = ctr[((i / D) - MD) * CC + (i % D) - MD];
#pragma unroll
        for (int t0 = 0; t0 < D * D; t0 += BG) {
#pragma unroll
            for (int i = 0; i < BG; ++i) {
                const int tn = t0 + BG + i;
                if (tn < D * D) nxt[i] = ctr[((tn / D) - MD) * CC + (tn % D) - MD];
            }
#pragma unroll
            for (int i = 0; i < BG; ++i) {
                const int tc = t0 + i;
                if (tc < D * D) {
                    s01 += pk_mul_bcast(tc & 1, wp[tc / 2], cur[i].xy);
                    s23 += pk_mul_bcast(tc & 1, wp[tc / 2], cur[i].zw);
                }
            }
            // the sums are used under `if (inimg)` only: without this anchor the adds are sunk there, behind all the products
            asm volatile("" : "+v"(s01), "+v"(s23));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < BG; ++i) cur[i] = nxt[i];
        }
        const f4 sum = (f4){s01.x, s01.y, s23.x, s23.y};
        if (inimg) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 4 * q + k;
                if (c < p.C) store_out(g + c * HW + y * p.W + x, (T)(sum[k] / nelems));
            }
        }
    }
}

// one batch item is indexed with ints, the grid's y / z extents are 16-bit
bool dense_fits(const CorrP &p)
{
    const long HW = (long)p.H * p.W;
    if (((long)p.C + 4) * HW >= (1L << 31) || (long)p.nOut * HW >= (1L << 31)) return false;   // C + 4: the zero-filled tail of the last quad
    if (p.B > 32767) return false;
    const long tiles = (long)((p.W + FTW - 1) / FTW) * ((p.H + FTH - 1) / FTH);
    return tiles < (1L << 31);
}

template <typename T, int MD>
int fwd_dense_launch(const void *in1, const void *in2, void *out, const CorrP &p, hipStream_t s)
{
    const int tilesX = (p.W + FTW - 1) / FTW, tilesY = (p.H + FTH - 1) / FTH;
    // two results of a lane go out as one store where every row of every plane keeps the pair aligned
    const int vec = (p.W % 2 == 0) && (p.out_bs % 2 == 0) && aligned(out, 2 * sizeof(T));
    hipLaunchKernelGGL((corr_fwd_dense<T, MD>), dim3(tilesX * tilesY, 1, p.B), dim3((2 * MD + 1) * 64), 0, s,
                       static_cast<const T *>(in1), static_cast<const T *>(in2), static_cast<T *>(out), p, tilesX, vec);
    return launch_status();
}

template <typename T, int MD>
int bwd_dense_launch(const void *in1, const void *in2, const void *gout, void *g1, void *g2, const CorrP &p, hipStream_t s)
{
    const int tilesX = (p.W + BTW - 1) / BTW, tilesY = (p.H + BTH - 1) / BTH;
    const int nq = (p.C + 3) / 4;
    // split the channels until about four workgroups per CU are in the grid (small maps, many channels)
    const long base = (long)tilesX * tilesY * p.B * 2;
    int split = (int)((1024 + base - 1) / base);
    if (split > nq) split = nq;
    if (split < 1) split = 1;
    const int qper = (nq + split - 1) / split;
    split = (nq + qper - 1) / qper;
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

bool corr_dense_applicable(int dtype, int C, int H, int W, int pad, int k, int md, int s1, int s2)
{
    (void)H; (void)W;
    return (dtype == FN2_F32 || dtype == FN2_F16 || dtype == FN2_BF16) && C >= 1 && k == 1 && s1 == 1 && s2 == 1 && pad == md &&
           md >= 1 && md <= DENSE_MAX_MD;
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

int corr_forward_dense(const void *in1, const void *in2, void *out, int dtype, const CorrP &p, hipStream_t s)
{
    if (!corr_dense_applicable(dtype, p.C, p.H, p.W, p.pad, p.k, p.md, p.s1, p.s2) || !dense_fits(p)) return FN2_EUNSUPPORTED;
    if (p.B == 0) return FN2_OK;
    switch (dtype) {
    case FN2_F32: return fwd_dense_md<float>(in1, in2, out, p, s);
    case FN2_F16: return fwd_dense_md<half_t>(in1, in2, out, p, s);
    case FN2_BF16: return fwd_dense_md<bf16_t>(in1, in2, out, p, s);
    default: return FN2_EUNSUPPORTED;
    }
}

int corr_backward_dense(const void *in1, const void *in2, const void *gout, void *g1, void *g2, int dtype, const CorrP &p,
                        hipStream_t s)
{
    if (!corr_dense_applicable(dtype, p.C, p.H, p.W, p.pad, p.k, p.md, p.s1, p.s2) || !dense_fits(p)) return FN2_EUNSUPPORTED;
    if (p.B == 0) return FN2_OK;
    switch (dtype) {
    case FN2_F32: return bwd_dense_md<float>(in1, in2, gout, g1, g2, p, s);
    case FN2_F16: return bwd_dense_md<half_t>(in1, in2, gout, g1, g2, p, s);
    case FN2_BF16: return bwd_dense_md<bf16_t>(in1, in2, gout, g1, g2, p, s);
    default: return FN2_EUNSUPPORTED;
    }
}

} // namespace fn2
