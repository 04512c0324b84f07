// capi_sample1d.hip -- C-ABI entry points of libflownet2_hip_sample1d.so (include/staging/flownet2_hip_sample1d.h): CorrSample1d.
// Self-contained: links nothing of the other libraries.  Every check comes before any launch, in the header's order.
#include "corr_sample1d.h"

extern "C" int fn2h_abi_version(void) { return FN2H_ABI_VERSION; }

namespace {
// checks 1 - 5 on what both entry points share; `ptrs` (the levels or their gradients) and W2 may be NULL until check 4.
// FN2_OK with p.B == 0 means "nothing to launch".
int make_params(fn2::Sample1dP &p, const void *const *ptrs, const int *W2, int num_levels, const void *a, const void *b, long long cbs,
                int B, int H, int W, int radius)
{
    if (num_levels < 1 || num_levels > FN2H_MAX_LEVELS || radius < 0 || radius > FN2H_MAX_RADIUS) return FN2_EINVAL;
    if (B < 0 || H < 1 || W < 1) return FN2_EINVAL;
    const long long lim = 0x7fffffffLL, plane = (long long)H * W;   // (each factor below 2^31: no product overflows 64 bits)
    if (cbs < plane) return FN2_EINVAL;
    if (W2)
        for (int l = 0; l < num_levels; ++l)
            if (W2[l] < 1) return FN2_EINVAL;
    if (plane > lim || B * plane > lim) return FN2_EUNSUPPORTED;
    const long long pixels = B * plane;
    if (W2)
        for (int l = 0; l < num_levels; ++l)
            if (pixels * W2[l] > (1LL << 48)) return FN2_EUNSUPPORTED;
    p = fn2::Sample1dP{};
    p.L = num_levels;
    p.B = B;
    p.H = H;
    p.W = W;
    p.r = radius;
    p.cbs = cbs;
    if (B == 0) return FN2_OK;
    if (!ptrs || !W2 || !a || !b) return FN2_EINVAL;
    for (int l = 0; l < num_levels; ++l)
        if (!ptrs[l]) return FN2_EINVAL;
    if (!fn2::aligned(a, 4) || !fn2::aligned(b, 4)) return FN2_EALIGN;
    for (int l = 0; l < num_levels; ++l) {
        if (!fn2::aligned(ptrs[l], 4)) return FN2_EALIGN;
        p.lvl[l] = static_cast<float *>(const_cast<void *>(ptrs[l]));
        p.W2[l] = W2[l];
    }
    return FN2_OK;
}
} // namespace

extern "C" int fn2h_corr_sample1d_forward(const void *const *levels, const int *W2, int num_levels, const void *coords_x,
                                          long long coords_batch_stride, void *out, int B, int H, int W, int radius, void *stream)
{
    fn2::Sample1dP p;
    const int rc = make_params(p, levels, W2, num_levels, coords_x, out, coords_batch_stride, B, H, W, radius);
    if (rc != FN2_OK || B == 0) return rc;
    return fn2::sample1d_forward(static_cast<const float *>(coords_x), static_cast<float *>(out), p, static_cast<hipStream_t>(stream));
}

extern "C" int fn2h_corr_sample1d_backward(const int *W2, int num_levels, const void *coords_x, long long coords_batch_stride,
                                           const void *grad_out, void *const *grad_levels, int B, int H, int W, int radius, void *stream)
{
    fn2::Sample1dP p;
    const int rc = make_params(p, grad_levels, W2, num_levels, coords_x, grad_out, coords_batch_stride, B, H, W, radius);
    if (rc != FN2_OK || B == 0) return rc;
    return fn2::sample1d_backward(static_cast<const float *>(coords_x), static_cast<const float *>(grad_out), p,
                                  static_cast<hipStream_t>(stream));
}
