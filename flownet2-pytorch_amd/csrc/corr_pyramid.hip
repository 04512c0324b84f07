// corr_pyramid.hip -- CorrPyramid (include/preview/flownet2_hip_pyramid.h): the build of RAFT's all-pairs correlation pyramid in one
// kernel, and the fold of the levels' gradients into the gradient of the volume.  gfx950 only.
//
// pyramid_fwd is a GEMM per batch item, M = H W queries x N = H2 W2 targets over K = C, on v_mfma_f32_32x32x16_bf16 through the
// exact three-term split of bf16x3.h (hh, hm, mh, hl, lh, mm: six products per fp32 product).  A workgroup of four waves owns TM =
// 128 queries and a TV x TU = 8 x 32 block of fmap2 aligned to 8 both ways; wave w owns queries 32 w .. 32 w + 31 against the whole
// block: eight 32 x 32 accumulators, one per fmap2 row of the block.  The D layout of the instruction puts the COLUMN on the lane
// (lane & 31) and 16 rows in the registers, so with the targets as columns a register is one query and the 32 lanes of a half wave
// are 32 consecutive target columns of that query's row: 128 contiguous bytes per store instruction and half wave, and the 2 x 2, 4
// x 4 and 8 x 8 pooling blocks are neighbouring lanes (columns) and neighbouring accumulators (rows) of the same lane.  Levels 1 .. 3
// come out of the registers the scale left the level-0 values in: nothing written is read back.
//
// Per 32 channels both operands are staged once: a lane loads 8 channels of one pixel (lanes = consecutive pixels: coalesced),
// splits them and writes three 16-byte fragments, one per term, into LDS rows of 64 bytes (32 bf16); the 16-byte slot of a row is
// XORed with (row >> 2) & 3, which makes both the staging writes and the operand reads (16 consecutive rows, one slot) touch every
// bank once.  Channels beyond C, queries beyond H W and targets outside fmap2 are staged as zeros; their outputs are masked.
#include "bf16x3.h"
#include "corr_pyramid.h"

namespace fn2 {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;                                               // four waves
constexpr int TM = FN2Y_TILE_QUERIES, TV = FN2Y_TILE_ROWS, TU = FN2Y_TILE_COLS, TN = TV * TU;
constexpr int KC = 32;                                                // channels per stage: two MFMA steps
constexpr int ROW = 2 * KC;                                           // bytes of an LDS row
constexpr int A_TERM = TM * ROW, B_TERM = TN * ROW;                   // bytes of one term's image
static_assert(TM == 4 * 32 && TU == 32 && TV == 8, "the epilogue below is written for four waves of 32 queries and 8 x 32 targets");

__device__ __forceinline__ int slot_offset(int row, int kg) { return row * ROW + ((kg ^ ((row >> 2) & 3)) << 4); }

// the value of lane ^ 1, ^ 2 (DPP quad_perm) and ^ 4 (ds_swizzle, bit mode) -- executed by every lane of the wave
__device__ __forceinline__ float lane_xor1(float x) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xf, 0xf, true)); }
__device__ __forceinline__ float lane_xor2(float x) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xf, 0xf, true)); }
__device__ __forceinline__ float lane_xor4(float x) { return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), 0x101F)); }

// 8 channels kg 8 .. kg 8 + 7 (from k0) of `rows` pixels each -> the three term images at `lds`; src(row) is the pixel's address in
// channel 0 of the batch item or nullptr for a pixel outside the map
template <int ROWS, int TERM, class Src>
__device__ __forceinline__ void stage(unsigned char *lds, int tid, int k0, int C, size_t plane, Src src)
{
#pragma unroll 2   // two items' 16 loads in flight; unrolled further the kernel spills at two workgroups per CU
    for (int it = 0; it < ROWS * 4 / NT; ++it) {
        const int i = tid + it * NT, row = i % ROWS, kg = i / ROWS;
        const float *g = src(row);
        float r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = k0 + kg * 8 + k;
            r[k] = (g && c < C) ? g[(size_t)c * plane] : 0.f;
        }
        u4 t0, t1, t2;
        split3(r, t0, t1, t2);
        const int off = slot_offset(row, kg);
        *reinterpret_cast<u4 *>(lds + off) = t0;
        *reinterpret_cast<u4 *>(lds + TERM + off) = t1;
        *reinterpret_cast<u4 *>(lds + 2 * TERM + off) = t2;
    }
}

__global__ __launch_bounds__(NT, 2) void pyramid_fwd(const float *__restrict__ f1, const float *__restrict__ f2, const PyramidP P,
                                                     const unsigned tilesU, const unsigned tilesN, const unsigned tilesM)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[3 * A_TERM + 3 * B_TERM];
    unsigned char *const ldsA = lds, *const ldsB = lds + 3 * A_TERM;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned nt = blockIdx.x % tilesN, rest = blockIdx.x / tilesN, mt = rest % tilesM, b = rest / tilesM;
    const int M = P.H * P.W, H2 = P.H2, W2 = P.W2, N = H2 * W2, C = P.C;   // M, N < 2^31
    const int m0 = (int)mt * TM, v0 = (int)(nt / tilesU) * TV, u0 = (int)(nt % tilesU) * TU;
    const float *f1b = f1 + (size_t)b * C * M, *f2b = f2 + (size_t)b * C * N;

    f16v acc[TV];
#pragma unroll
    for (int j = 0; j < TV; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    auto as_bf = [](const u4 &x) { return __builtin_bit_cast(bf16x8, x); };
    const int col = lane & 31, half = lane >> 5;

    for (int k0 = 0; k0 < C; k0 += KC) {
        if (k0) __syncthreads();   // the last stage's operand reads are done
        stage<TM, A_TERM>(ldsA, tid, k0, C, (size_t)M, [&](int row) { return m0 + row < M ? f1b + m0 + row : nullptr; });
        stage<TN, B_TERM>(ldsB, tid, k0, C, (size_t)N, [&](int row) {
            const int v = v0 + row / TU, u = u0 + row % TU;
            return (v < H2 && u < W2) ? f2b + (size_t)v * W2 + u : nullptr;
        });
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KC / 16; ++ks) {
            const int kg = 2 * ks + half;   // this lane's 8 channels of the step
            const int offA = slot_offset(wave * 32 + col, kg);
            const u4 a0 = *reinterpret_cast<const u4 *>(ldsA + offA), a1 = *reinterpret_cast<const u4 *>(ldsA + A_TERM + offA),
                     a2 = *reinterpret_cast<const u4 *>(ldsA + 2 * A_TERM + offA);
#pragma unroll
            for (int j = 0; j < TV; ++j) {
                const int offB = slot_offset(j * TU + col, kg);
                const u4 b0 = *reinterpret_cast<const u4 *>(ldsB + offB), b1 = *reinterpret_cast<const u4 *>(ldsB + B_TERM + offB),
                         b2 = *reinterpret_cast<const u4 *>(ldsB + 2 * B_TERM + offB);
                // D[query][target] += A[query][k] B[k][target]; the small terms first
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(a1), as_bf(b1), acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(a0), as_bf(b2), acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(a2), as_bf(b0), acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(a0), as_bf(b1), acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(a1), as_bf(b0), acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(a0), as_bf(b0), acc[j], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: register r of accumulator j is query (r & 3) + 8 (r >> 2) + 4 half of the wave's 32, target (v0 + j, u0 + col)
    const int L = P.L, u = u0 + col;
    const int H1 = H2 >> 1, W1 = W2 >> 1, H2b = H2 >> 2, W2b = W2 >> 2, H3 = H2 >> 3, W3 = W2 >> 3;
    const float s = P.s;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int q = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool qok = q < M;
        const size_t p = (size_t)b * M + (qok ? q : 0);
        float x0[TV];
#pragma unroll
        for (int j = 0; j < TV; ++j) x0[j] = acc[j][r] * s;
        if (qok && u < W2) {
            float *d = P.lvl[0] + p * (size_t)N + (size_t)v0 * W2 + u;
#pragma unroll
            for (int j = 0; j < TV; ++j)
                if (v0 + j < H2) store_out(d + j * W2, x0[j]);
        }
        if (L < 2) continue;
        float x1[TV / 2];
#pragma unroll
        for (int j = 0; j < TV / 2; ++j) {
            const float top = x0[2 * j] + lane_xor1(x0[2 * j]), bottom = x0[2 * j + 1] + lane_xor1(x0[2 * j + 1]);
            x1[j] = (top + bottom) * 0.25f;
        }
        if (qok && !(col & 1) && (u >> 1) < W1) {
            float *d = P.lvl[1] + p * ((size_t)H1 * W1) + (size_t)(v0 >> 1) * W1 + (u >> 1);
#pragma unroll
            for (int j = 0; j < TV / 2; ++j)
                if ((v0 >> 1) + j < H1) store_out(d + j * W1, x1[j]);
        }
        if (L < 3) continue;
        float x2[TV / 4];
#pragma unroll
        for (int j = 0; j < TV / 4; ++j) {
            const float top = x1[2 * j] + lane_xor2(x1[2 * j]), bottom = x1[2 * j + 1] + lane_xor2(x1[2 * j + 1]);
            x2[j] = (top + bottom) * 0.25f;
        }
        if (qok && !(col & 3) && (u >> 2) < W2b) {
            float *d = P.lvl[2] + p * ((size_t)H2b * W2b) + (size_t)(v0 >> 2) * W2b + (u >> 2);
#pragma unroll
            for (int j = 0; j < TV / 4; ++j)
                if ((v0 >> 2) + j < H2b) store_out(d + j * W2b, x2[j]);
        }
        if (L < 4) continue;
        const float top = x2[0] + lane_xor4(x2[0]), bottom = x2[1] + lane_xor4(x2[1]);
        const float x3 = (top + bottom) * 0.25f;
        if (qok && !(col & 7) && (u >> 3) < W3 && (v0 >> 3) < H3)
            store_out(P.lvl[3] + p * ((size_t)H3 * W3) + (size_t)(v0 >> 3) * W3 + (u >> 3), x3);
    }
}

// One lane per four consecutive columns of one level-0 row; VEC: W2 % 4 == 0 and g0 (where given) and G 16-byte aligned.
template <bool VEC> __global__ __launch_bounds__(NT) void pyramid_fold_kernel(const PyramidP P, float *__restrict__ G)
{
    const unsigned H2 = P.H2, W2 = P.W2, W4 = (W2 + 3) / 4;
    const size_t total = (size_t)P.B * P.H * P.W * H2 * W4, stride = (size_t)gridDim.x * NT;
    const float *g0 = P.lvl[0];
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += stride) {
        const unsigned u = 4 * (unsigned)(i % W4);
        const size_t row = i / W4, p = row / H2;
        const unsigned v = (unsigned)(row % H2), n = W2 - u < 4 ? W2 - u : 4;
        const size_t base = row * W2 + u;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (g0) {
            if constexpr (VEC) {
                const f4 x = *reinterpret_cast<const f4 *>(g0 + base);
#pragma unroll
                for (int k = 0; k < 4; ++k) a[k] = x[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if ((unsigned)k < n) a[k] = g0[base + k];
            }
        }
#pragma unroll
        for (int l = 1; l < FN2Y_MAX_LEVELS; ++l) {
            if (l >= P.L || !P.lvl[l]) continue;
            const unsigned Hl = H2 >> l, Wl = W2 >> l;
            if ((v >> l) >= Hl) continue;
            const float *gl = P.lvl[l] + (p * Hl + (v >> l)) * Wl;
            const float w = l == 1 ? 0.25f : l == 2 ? 0.0625f : 0.015625f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((unsigned)k < n && ((u + k) >> l) < Wl) a[k] = a[k] + w * gl[(u + k) >> l];
        }
        if constexpr (VEC) {
            f4 y;
#pragma unroll
            for (int k = 0; k < 4; ++k) y[k] = P.s * a[k];
            store_out(reinterpret_cast<f4 *>(G + base), y);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((unsigned)k < n) store_out(G + base + k, P.s * a[k]);
        }
    }
}

} // namespace

int pyramid_forward(const float *f1, const float *f2, const PyramidP &p, hipStream_t s)
{
    const size_t tilesU = ((size_t)p.W2 + TU - 1) / TU, tilesN = (((size_t)p.H2 + TV - 1) / TV) * tilesU;
    const size_t tilesM = ((size_t)p.H * p.W + TM - 1) / TM, blocks = (size_t)p.B * tilesM * tilesN;
    if (blocks > 0x7fffffffULL) return FN2_EUNSUPPORTED;
    hipLaunchKernelGGL(pyramid_fwd, dim3((unsigned)blocks), dim3(NT), 0, s, f1, f2, p, (unsigned)tilesU, (unsigned)tilesN, (unsigned)tilesM);
    return launch_status();
}

int pyramid_fold(const PyramidP &p, float *G, hipStream_t s)
{
    const size_t total = (size_t)p.B * p.H * p.W * p.H2 * (((size_t)p.W2 + 3) / 4), want = (total + NT - 1) / NT;
    const unsigned blocks = (unsigned)(want < 0x7fffffffULL ? want : 0x7fffffffULL);
    const bool vec = p.W2 % 4 == 0 && aligned(G, 16) && (!p.lvl[0] || aligned(p.lvl[0], 16));
    if (vec) hipLaunchKernelGGL(pyramid_fold_kernel<true>, dim3(blocks), dim3(NT), 0, s, p, G);
    else hipLaunchKernelGGL(pyramid_fold_kernel<false>, dim3(blocks), dim3(NT), 0, s, p, G);
    return launch_status();
}

} // namespace fn2
