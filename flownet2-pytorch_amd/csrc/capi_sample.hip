// capi_sample.hip -- C-ABI entry points of libflownet2_hip_sample.so (include/preview/flownet2_hip_sample.h): CorrSample.
// Self-contained: links nothing of the other libraries.  Every check comes before any launch, in the header's order.
#include "corr_sample.h"

extern "C" int fn2p_abi_version(void) { return FN2P_ABI_VERSION; }

namespace {
// checks 1 - 4 on what both entry points share; `ptrs` (the levels or their gradients) and the size arrays may be NULL until
// check 4.  FN2_OK with p.B == 0 means "nothing to launch".
int make_params(fn2::SampleP &p, const void *const *ptrs, const int *H2, const int *W2, int num_levels, const void *a, const void *b,
                int B, int H, int W, int radius)
{
    if (num_levels < 1 || num_levels > FN2P_MAX_LEVELS || radius < 0 || radius > FN2P_MAX_RADIUS) return FN2_EINVAL;
    if (B < 0 || H < 1 || W < 1) return FN2_EINVAL;
    const bool sized = H2 && W2;
    if (sized)
        for (int l = 0; l < num_levels; ++l)
            if (H2[l] < 1 || W2[l] < 1) return FN2_EINVAL;
    const long long lim = 0x7fffffffLL, plane = (long long)H * W;
    if (plane > lim || B * plane > lim) return FN2_EUNSUPPORTED;   // (each factor below 2^31: no product overflows 64 bits)
    const long long pixels = B * plane;
    if (sized)
        for (int l = 0; l < num_levels; ++l) {
            const long long slice = (long long)H2[l] * W2[l];
            if (slice > lim || pixels * slice > (1LL << 48)) return FN2_EUNSUPPORTED;
        }
    p = fn2::SampleP{};
    p.L = num_levels;
    p.B = B;
    p.H = H;
    p.W = W;
    p.r = radius;
    if (B == 0) return FN2_OK;
    if (!ptrs || !sized || !a || !b) return FN2_EINVAL;
    for (int l = 0; l < num_levels; ++l)
        if (!ptrs[l]) return FN2_EINVAL;
    if (!fn2::aligned(a, 4) || !fn2::aligned(b, 4)) return FN2_EALIGN;
    for (int l = 0; l < num_levels; ++l) {
        if (!fn2::aligned(ptrs[l], 4)) return FN2_EALIGN;
        p.lvl[l] = static_cast<float *>(const_cast<void *>(ptrs[l]));
        p.H2[l] = H2[l];
        p.W2[l] = W2[l];
    }
    return FN2_OK;
}
} // namespace

extern "C" int fn2p_corr_sample_forward(const void *const *levels, const int *H2, const int *W2, int num_levels, const void *coords,
                                        void *out, int B, int H, int W, int radius, void *stream)
{
    fn2::SampleP p;
    const int rc = make_params(p, levels, H2, W2, num_levels, coords, out, B, H, W, radius);
    if (rc != FN2_OK || B == 0) return rc;
    return fn2::sample_forward(static_cast<const float *>(coords), static_cast<float *>(out), p, static_cast<hipStream_t>(stream));
}

extern "C" int fn2p_corr_sample_backward(const int *H2, const int *W2, int num_levels, const void *coords, const void *grad_out,
                                         void *const *grad_levels, int B, int H, int W, int radius, void *stream)
{
    fn2::SampleP p;
    const int rc = make_params(p, grad_levels, H2, W2, num_levels, coords, grad_out, B, H, W, radius);
    if (rc != FN2_OK || B == 0) return rc;
    return fn2::sample_backward(static_cast<const float *>(coords), static_cast<const float *>(grad_out), p,
                                static_cast<hipStream_t>(stream));
}
