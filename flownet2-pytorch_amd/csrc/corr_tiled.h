// corr_tiled.h -- the channel-quad tiling of the LDS-tiled correlation kernels, shared by the dense 2-D kernels
// (correlation_dense.hip, libflownet2_hip.so) and the 1-D ones (correlation_1d.hip, libflownet2_hip_ext.so): one definition of
// every piece both use, so the two cannot drift apart.  The libraries do not link each other; this header knows neither CorrP nor
// Corr1dP.  A kernel keeps what is its own: which pixel a staged slot holds and where it lies in LDS, the gO factors of a lane,
// the output addressing and the rule for when a term is absent.
//
// The tiling: a workgroup owns one batch item and a tile of pixels and walks the channels four at a time.  The four channels of
// one pixel are staged side by side (16 bytes for fp32 / bf16-as-fp32, 8 bytes for half), so every LDS read is one aligned
// ds_read_b128 / b64 whatever the displacement, and the four lanes of the vector are the forward's four chains.  The next four
// channels travel from global memory into registers while the current ones are multiplied (two LDS buffers, one barrier per step).
#pragma once
#include "corr_arith.h"

namespace fn2 {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int FTW = 32, FTH = 4;   // forward tile (pixels)
constexpr int BTW = 32, BTH = 8;   // backward tile
constexpr int BG = 3;              // backward: displacements per scheduling group

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

// ---------------------------------------------------------------- staging
// What one lane of NT stages of every channel quad: slot i is pixel e = tid + i * NT of the workgroup's LDS image.  The kernel
// fills src / goff / lidx once (its own mapping from e to a tensor, an image pixel and an LDS index); load() and step() are the
// pipeline.  L is the LDS element type, C and HW the channels and the plane size of the tensors in src.
template <typename T, typename L, int NLD, int NT> struct QuadStage {
    typedef L l4 __attribute__((ext_vector_type(4)));
    const T *src[NLD];
    int goff[NLD];   // the pixel's offset in its plane; -1 = outside the image (zero)
    int lidx[NLD];   // where it goes in the LDS image; -1 = a slot past the image's end (nothing is written)
    T val[NLD][4];   // the four channels of slot i as they were loaded
    int C, HW;

    // quad q sets out from global memory: always a load from inside the tensor (the address is clamped; no branch around it).
    // The values stay as loaded until step() converts and selects: either would need them at once, and the round trip through
    // memory would stand in front of the products instead of under them.
    __device__ __forceinline__ void load(int q)
    {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
#pragma unroll
            for (int k = 0; k < 4; ++k) val[i][k] = src[i][max(goff[i], 0) + min(4 * q + k, C - 1) * HW];
        }
    }

    // quad q, loaded, goes into `buf` (the LDS buffer of its parity), zero where the pixel or the channel does not exist, while
    // quad q + 1 sets out
    __device__ __forceinline__ void step(l4 *buf, int q, int qend)
    {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            l4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k)   // & and not &&: a select, not a branch
                v[k] = ((goff[i] >= 0) & (4 * q + k < C)) ? (L)val[i][k] : (L)0.0f;
            if (lidx[i] >= 0) buf[lidx[i]] = v;
        }
        __syncthreads();   // the only barrier of a step: the buffer written next was last read before this one
        if (q + 1 < qend) load(q + 1);
    }
};

// ---------------------------------------------------------------- forward
// The products of one channel quad: acc[px][d] (component = chain, channel mod 4) of the lane's two adjacent in1 pixels at
// buf[offA], buf[offA + 1] and ND displacements, pixel px against buf[offB + d + px].  full: all four channels exist; otherwise
// the C % 4 = rem leftover channels go to the first chain, in order.
template <typename L, int ND, typename V>
__device__ __forceinline__ void fwd_quad(f4 (&acc)[2][ND], const V *buf, int offA, int offB, bool full, int rem)
{
    const V a0 = buf[offA], a1 = buf[offA + 1];
    V bv[ND + 1];
#pragma unroll
    for (int j = 0; j < ND + 1; ++j) bv[j] = buf[offB + j];
    if (full) {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                const V av = px ? a1 : a0;
                const V w = bv[d + px];
                f4 pr;
#pragma unroll
                for (int k = 0; k < 4; ++k) pr[k] = fwd_prod<L>(av[k], w[k]);
                acc[px][d] += pr;
            }
        }
    } else {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                const V av = px ? a1 : a0;
                const V w = bv[d + px];
                float s0 = acc[px][d][0];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < rem) s0 += fwd_prod<L>(av[k], w[k]);
                acc[px][d][0] = s0;
            }
        }
    }
}

// the sum of one (pixel, displacement) pair from its four chains; a pair whose in2 pixel lies outside the image is absent
__device__ __forceinline__ float fwd_lane_sum(f4 s, bool present)
{
    float sum = 0.0f;
    sum += (s[0] + s[1]) + (s[2] + s[3]);
    if (!present) sum = 0.0f;   // absent, not zero-multiplied (the sum may be NaN from inf * 0 on the zero-filled halo)
    return sum;
}

// the two results of a lane: one store where the launch found every pair aligned (fwd_pairs_aligned), else one by one
template <typename T> __device__ __forceinline__ void store_results(T *od, const T (&res2)[2], int vec, bool second)
{
    if (vec) {
        store_pair<T>(od, res2[0], res2[1]);
    } else {
        store_out(od, res2[0]);
        if (second) store_out(od + 1, res2[1]);
    }
}

// ---------------------------------------------------------------- backward
// One channel quad of one pixel: the sequential sums over displacements t = 0 .. n - 1 of wp[t] * ctr[off(t)], the gO factor t
// being half t & 1 of pair wp[t / 2].  N >= n is the compile-time slot count; where n is a runtime value the groups and
// displacements from n on are skipped by wave-uniform branches, where it is N they fold away.
template <int N, typename Off>
__device__ __forceinline__ f4 bwd_quad(const f4 *ctr, const f2 (&wp)[(N + 1) / 2], int n, Off off)
{
    f2 s01 = (f2){0.0f, 0.0f}, s23 = (f2){0.0f, 0.0f};
    // BG displacements at a time, the reads of the next group in flight: left alone, the scheduler forms every product first
    // (they are independent, the two sums are chains) and spills them
    f4 cur[BG], nxt[BG];
#pragma unroll
    for (int i = 0; i < BG; ++i) cur[i] = ctr[off(i)];
#pragma unroll
    for (int t0 = 0; t0 < N; t0 += BG) {
        if (t0 < n) {
#pragma unroll
            for (int i = 0; i < BG; ++i) {
                const int tn = t0 + BG + i;
                if (tn < N) nxt[i] = ctr[off(tn)];
            }
#pragma unroll
            for (int i = 0; i < BG; ++i) {
                const int t = t0 + i;
                if (t < N && t < n) {
                    s01 += pk_mul_bcast(t & 1, wp[t / 2], cur[i].xy);
                    s23 += pk_mul_bcast(t & 1, wp[t / 2], cur[i].zw);
                }
            }
            // the sums are used under `if (inimg)` only: without this anchor the adds are sunk there, behind all the products
            asm volatile("" : "+v"(s01), "+v"(s23));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < BG; ++i) cur[i] = nxt[i];
        }
    }
    return (f4){s01.x, s01.y, s23.x, s23.y};
}

// the four channels of quad q of one pixel (g: the pixel in channel 0's plane), / nelems, rounded once to T
template <typename T> __device__ __forceinline__ void bwd_store_quad(T *g, int pix, int q, int C, int HW, f4 sum, float nelems)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 4 * q + k;
        if (c < C) store_out(g + c * HW + pix, (T)(sum[k] / nelems));
    }
}

// ---------------------------------------------------------------- host
// one batch item is indexed with ints, the grid's y / z extents are 16-bit
template <typename P> bool tiled_fits(const P &p)
{
    const long HW = (long)p.H * p.W;
    if (((long)p.C + 4) * HW >= (1L << 31) || (long)p.nOut * HW >= (1L << 31)) return false;   // C + 4: the zero-filled tail of the last quad
    if (p.B > 32767) return false;
    const long tiles = (long)((p.W + FTW - 1) / FTW) * ((p.H + FTH - 1) / FTH);
    return tiles < (1L << 31);
}

// forward: two results of a lane go out as one store where every row of every plane keeps the pair aligned
inline int fwd_pairs_aligned(int W, long out_bs, const void *out, size_t elem)
{
    return (W % 2 == 0) && (out_bs % 2 == 0) && aligned(out, 2 * elem);
}

// backward: split the nq channel quads until about four workgroups per CU are in the grid (small maps, many channels), `base`
// being the workgroups of one split; returns the quads per workgroup, *split = the grid's y extent
inline int bwd_channel_split(long base, int nq, int *split)
{
    int n = (int)((1024 + base - 1) / base);
    if (n > nq) n = nq;
    if (n < 1) n = 1;
    const int qper = (nq + n - 1) / n;
    *split = (nq + qper - 1) / qper;
    return qper;
}

} // namespace fn2
