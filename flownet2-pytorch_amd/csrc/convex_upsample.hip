// convex_upsample.hip -- ConvexUpsample (include/flownet2_hip_upsample.h): RAFT's convex flow upsampling, forward and backward,
// gfx950.  Memory-bound: the mask (9 f^2 planes) is read once per direction, coalesced along x with one lane per pixel; what is
// contiguous along f x + j instead (out, grad_out) goes through LDS as whole rows of FN2U_TILE f floats.  No atomics.
//
// A workgroup owns FN2U_TILE pixels of one row and has G = FN2U_GROUPS(f) waves; wave w takes the sub-rows i = w, w + G, ...
// (the same number for every wave, so the barriers are uniform).  The 3 x 3 flow neighbourhood of a pixel, scaled, lives in
// registers (9 C values); the arithmetic order is the header's.
#include "convex_upsample.h"
#include "../../include/flownet2_hip_upsample.h"

namespace fn2 {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int TILE = FN2U_TILE;
static_assert(TILE == FN2_WAVE, "one lane per pixel of the tile");

__device__ __forceinline__ float widen(float m) { return m; }
__device__ __forceinline__ float widen(half_t m) { return (float)m; }
__device__ __forceinline__ float widen(bf16_t m) { return __builtin_bit_cast(float, (unsigned)__builtin_bit_cast(unsigned short, m) << 16); }
// the fp32 value rounded to nearest even, once.  The empty asm keeps the product that made g an fp32 instruction of its own:
// without it the compiler folds multiply and conversion into v_fma_mixlo_f16, which rounds the exact product to float16
// directly and differs from the float32 call's gradient, rounded, in about one element in ten thousand.
template <class M> __device__ __forceinline__ M narrow(float g)
{
    asm volatile("" : "+v"(g));
    return (M)g;
}

// the block's place: tile of the row, row, batch item
struct Place {
    int b, y, x0, lane, w, npix, xc;
    bool valid;
};
__device__ __forceinline__ Place place(const UpsampleP &p)
{
    Place q;
    const unsigned row = blockIdx.x / (unsigned)p.tiles;
    q.x0 = (int)(blockIdx.x % (unsigned)p.tiles) * TILE;
    q.y = (int)(row % (unsigned)p.H);
    q.b = (int)(row / (unsigned)p.H);
    q.lane = threadIdx.x & (FN2_WAVE - 1);
    q.w = threadIdx.x / FN2_WAVE;
    q.npix = min(TILE, p.W - q.x0);
    q.valid = q.lane < q.npix;
    q.xc = min(q.x0 + q.lane, p.W - 1);   // lanes beyond the row work on its last pixel and store nothing
    return q;
}

// v[c][k] = scale * flow[b, c, y + ky - 1, x + kx - 1]; +0 for a tap outside the image (every load is clamped into the tensor)
template <int C> __device__ __forceinline__ void load_taps(const float *__restrict__ flow, const UpsampleP &p, const Place &q, float (&v)[C][9])
{
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float *pl = flow + (size_t)(q.b * C + c) * p.H * p.W;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = q.y + k / 3 - 1, xx = q.xc + k % 3 - 1;
            const bool in = yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
            const float t = p.scale * pl[(size_t)min(max(yy, 0), p.H - 1) * p.W + min(max(xx, 0), p.W - 1)];
            v[c][k] = in ? t : 0.f;
        }
    }
}

// the nine weights of sub-position `sub` = i f + j; mp points at the pixel in mask channel 0 of its batch item
template <int F, class M> __device__ __forceinline__ void softmax9(const M *__restrict__ mp, size_t HW, int sub, float (&pk)[9])
{
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = widen(mp[(size_t)(k * F * F + sub) * HW]);
    float mx = m[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, m[k]);
    float e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = expf(m[k] - mx);
    float s = e[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) s = s + e[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) pk[k] = e[k] / s;
}

// whole rows of n floats between global memory and an LDS row: 16 bytes per lane where the global row starts on a 16-byte
// boundary (wave-uniform), single floats where it does not and for the last n % 4
__device__ __forceinline__ void store_row(float *__restrict__ rowp, const float *src, int n, int lane)
{
    if ((reinterpret_cast<uintptr_t>(rowp) & 15) == 0) {
        const int nq = n >> 2;
        for (int q = lane; q < nq; q += FN2_WAVE) __builtin_nontemporal_store(*reinterpret_cast<const f4 *>(src + 4 * q), reinterpret_cast<f4 *>(rowp) + q);
        for (int e = (nq << 2) + lane; e < n; e += FN2_WAVE) rowp[e] = src[e];
    } else {
        for (int e = lane; e < n; e += FN2_WAVE) rowp[e] = src[e];
    }
}
__device__ __forceinline__ void load_row(const float *__restrict__ rowp, float *dst, int n, int lane)
{
    if ((reinterpret_cast<uintptr_t>(rowp) & 15) == 0) {
        const int nq = n >> 2;
        for (int q = lane; q < nq; q += FN2_WAVE) *reinterpret_cast<f4 *>(dst + 4 * q) = reinterpret_cast<const f4 *>(rowp)[q];
        for (int e = (nq << 2) + lane; e < n; e += FN2_WAVE) dst[e] = rowp[e];
    } else {
        for (int e = lane; e < n; e += FN2_WAVE) dst[e] = rowp[e];
    }
}

// row f y + i of channel c of batch item b in a B x C x f H x f W tensor, from the tile's first column on
template <int F, int C> __device__ __forceinline__ size_t up_row(const UpsampleP &p, const Place &q, int c, int i)
{
    return ((size_t)(q.b * C + c) * (F * p.H) + (F * q.y + i)) * (size_t)(F * p.W) + (size_t)F * q.x0;
}

template <int F, int C, class M>
__global__ __launch_bounds__(FN2_WAVE *FN2U_GROUPS(F)) void convex_upsample_fwd(const float *__restrict__ flow, const M *__restrict__ mask,
                                                                                 float *__restrict__ out, const UpsampleP p)
{
    constexpr int G = FN2U_GROUPS(F), ROW = TILE * F;
    __shared__ __attribute__((aligned(16))) float slab[G][C * ROW];   // per wave: one output row per channel
    const Place q = place(p);
    const size_t HW = (size_t)p.H * p.W;
    float v[C][9];
    load_taps<C>(flow, p, q, v);
    const M *mp = mask + (size_t)q.b * (9 * F * F) * HW + (size_t)q.y * p.W + q.xc;
    float *sw = slab[q.w];
    for (int i = q.w; i < F; i += G) {
        float r[C][F];
#pragma unroll
        for (int j = 0; j < F; ++j) {
            float pk[9];
            softmax9<F>(mp, HW, i * F + j, pk);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 9; ++k) acc = acc + pk[k] * v[c][k];
                r[c][j] = acc;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {   // the lane's f results, contiguous in the row
            float *d = sw + c * ROW + q.lane * F;
            if constexpr (F == 2) *reinterpret_cast<f2 *>(d) = f2{r[c][0], r[c][1]};
            else {
#pragma unroll
                for (int j = 0; j < F; j += 4) *reinterpret_cast<f4 *>(d + j) = f4{r[c][j], r[c][j + 1], r[c][j + 2], r[c][j + 3]};
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; ++c) store_row(out + up_row<F, C>(p, q, c, i), sw + c * ROW, q.npix * F, q.lane);
        __syncthreads();
    }
}

// grad_mask and T[b, c, k, y, x] = sum_{i,j} p_k gO_c in the header's order
template <int F, int C, class M>
__global__ __launch_bounds__(FN2_WAVE *FN2U_GROUPS(F)) void convex_upsample_bwd_mask(const float *__restrict__ flow, const M *__restrict__ mask,
                                                                                      const float *__restrict__ go, M *__restrict__ gmask,
                                                                                      float *__restrict__ T, const UpsampleP p)
{
    constexpr int G = FN2U_GROUPS(F), ROW = TILE * F;
    constexpr int SLAB = G * C * ROW, RED = G * C * 9 * TILE;
    // per wave one grad_out row per channel; afterwards the groups' partial sums of T
    __shared__ __attribute__((aligned(16))) float lds[SLAB > RED ? SLAB : RED];
    const Place q = place(p);
    const size_t HW = (size_t)p.H * p.W;
    float v[C][9];
    load_taps<C>(flow, p, q, v);
    const size_t pix = (size_t)q.b * (9 * F * F) * HW + (size_t)q.y * p.W + q.xc;
    const M *mp = mask + pix;
    M *gp = gmask + pix;
    float *sw = lds + q.w * C * ROW;
    float acc[C][9];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[c][k] = 0.f;
    for (int i = q.w; i < F; i += G) {
#pragma unroll
        for (int c = 0; c < C; ++c) load_row(go + up_row<F, C>(p, q, c, i), sw + c * ROW, q.npix * F, q.lane);
        __syncthreads();
        float g[C][F];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int j = 0; j < F; ++j) g[c][j] = q.valid ? sw[c * ROW + q.lane * F + j] : 0.f;
#pragma unroll
        for (int j = 0; j < F; ++j) {
            float pk[9], d[9];
            softmax9<F>(mp, HW, i * F + j, pk);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float t = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) t = t + g[c][j] * v[c][k];
                d[k] = t;
            }
            float dbar = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) dbar = dbar + pk[k] * d[k];
            if (q.valid) {
#pragma unroll
                for (int k = 0; k < 9; ++k) gp[(size_t)(k * F * F + i * F + j) * HW] = narrow<M>(pk[k] * (d[k] - dbar));
            }
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[c][k] = acc[c][k] + pk[k] * g[c][j];
        }
        __syncthreads();
    }
    // the groups' sums, added in ascending order
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) lds[((q.w * C + c) * 9 + k) * TILE + q.lane] = acc[c][k];
    __syncthreads();
    for (int idx = threadIdx.x; idx < C * 9 * TILE; idx += FN2_WAVE * G) {
        const int ck = idx / TILE, l = idx % TILE;
        float t = lds[ck * TILE + l];
#pragma unroll
        for (int w = 1; w < G; ++w) t = t + lds[(w * C * 9 + ck) * TILE + l];
        if (l < q.npix) T[((size_t)q.b * (C * 9) + ck) * HW + (size_t)q.y * p.W + q.x0 + l] = t;
    }
}

// grad_flow[b, c, y', x'] = scale * sum over ascending k of T[b, c, k, y' - ky + 1, x' - kx + 1], pixels outside the image left out
__global__ __launch_bounds__(256) void convex_upsample_bwd_flow(const float *__restrict__ T, float *__restrict__ gflow, const UpsampleP p)
{
    const size_t HW = (size_t)p.H * p.W, total = (size_t)p.B * p.C * HW;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t bc = e / HW;
        const int yx = (int)(e % HW), y = yx / p.W, x = yx % p.W;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y - k / 3 + 1, xx = x - k % 3 + 1;
            if (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) s = s + T[(bc * 9 + k) * HW + (size_t)yy * p.W + xx];
        }
        gflow[e] = p.scale * s;
    }
}

template <int F, int C, class M> int launch_fwd(const float *flow, const void *mask, float *out, const UpsampleP &p, hipStream_t s)
{
    const unsigned blocks = (unsigned)p.B * p.H * p.tiles;
    hipLaunchKernelGGL((convex_upsample_fwd<F, C, M>), dim3(blocks), dim3(FN2_WAVE * FN2U_GROUPS(F)), 0, s, flow, static_cast<const M *>(mask), out, p);
    return launch_status();
}
template <int F, int C, class M>
int launch_bwd(const float *flow, const void *mask, const float *go, void *gmask, float *T, const UpsampleP &p, hipStream_t s)
{
    const unsigned blocks = (unsigned)p.B * p.H * p.tiles;
    hipLaunchKernelGGL((convex_upsample_bwd_mask<F, C, M>), dim3(blocks), dim3(FN2_WAVE * FN2U_GROUPS(F)), 0, s, flow, static_cast<const M *>(mask), go,
                       static_cast<M *>(gmask), T, p);
    return launch_status();
}

// (factor, channels, mask type) -> instantiation
#define FN2U_BY_C(CALL, F, M)                 \
    switch (p.C) {                            \
    case 1: return CALL<F, 1, M>;             \
    case 2: return CALL<F, 2, M>;             \
    case 3: return CALL<F, 3, M>;             \
    case 4: return CALL<F, 4, M>;             \
    default: return nullptr;                  \
    }
#define FN2U_BY_F(CALL, M)                    \
    switch (p.f) {                            \
    case 2: FN2U_BY_C(CALL, 2, M)             \
    case 4: FN2U_BY_C(CALL, 4, M)             \
    case 8: FN2U_BY_C(CALL, 8, M)             \
    default: return nullptr;                  \
    }
#define FN2U_PICK(CALL)                                 \
    switch (mask_dtype) {                               \
    case FN2_F32: FN2U_BY_F(CALL, float)                \
    case FN2_F16: FN2U_BY_F(CALL, half_t)               \
    case FN2_BF16: FN2U_BY_F(CALL, bf16_t)              \
    default: return nullptr;                            \
    }

typedef int (*FwdFn)(const float *, const void *, float *, const UpsampleP &, hipStream_t);
typedef int (*BwdFn)(const float *, const void *, const float *, void *, float *, const UpsampleP &, hipStream_t);
FwdFn pick_fwd(int mask_dtype, const UpsampleP &p) { FN2U_PICK(launch_fwd) }
BwdFn pick_bwd(int mask_dtype, const UpsampleP &p) { FN2U_PICK(launch_bwd) }

} // namespace

int upsample_make_params(UpsampleP &p, int B, int C, int H, int W, int factor, float scale)
{
    if (factor != 2 && factor != 4 && factor != 8) return FN2_EINVAL;
    if (B < 0 || C < 1 || H < 1 || W < 1) return FN2_EINVAL;
    if (C > FN2U_MAX_CHANNELS) return FN2_EUNSUPPORTED;
    // an output plane, and the number of workgroups, within 31 bits (H W < 2^62; after the first test H tiles <= H W < 2^29)
    const unsigned long long hw = (unsigned long long)H * (unsigned long long)W;
    if (hw >= (1ull << 31) / (unsigned)(factor * factor)) return FN2_EUNSUPPORTED;
    const int tiles = (W + FN2U_TILE - 1) / FN2U_TILE;
    if ((unsigned long long)B * H * tiles >= (1ull << 31)) return FN2_EUNSUPPORTED;
    p = UpsampleP{B, C, H, W, factor, tiles, scale};
    return FN2_OK;
}

int upsample_forward(const float *flow, const void *mask, float *out, int mask_dtype, const UpsampleP &p, hipStream_t s)
{
    FwdFn fn = pick_fwd(mask_dtype, p);
    return fn ? fn(flow, mask, out, p, s) : FN2_EINVAL;
}

int upsample_backward(const float *flow, const void *mask, const float *go, float *gflow, void *gmask, float *T, int mask_dtype,
                      const UpsampleP &p, hipStream_t s)
{
    BwdFn fn = pick_bwd(mask_dtype, p);
    if (!fn) return FN2_EINVAL;
    int rc = fn(flow, mask, go, gmask, T, p, s);
    if (rc != FN2_OK) return rc;
    const size_t total = (size_t)p.B * p.C * p.H * p.W;
    const size_t want = (total + 255) / 256;
    hipLaunchKernelGGL(convex_upsample_bwd_flow, dim3((unsigned)(want < (1u << 20) ? want : (1u << 20))), dim3(256), 0, s, T, gflow, p);
    return launch_status();
}

} // namespace fn2
