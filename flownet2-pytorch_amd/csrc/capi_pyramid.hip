// capi_pyramid.hip -- C-ABI entry points of libflownet2_hip_pyramid.so (include/preview/flownet2_hip_pyramid.h): CorrPyramid.
// Self-contained: links nothing of the other libraries.  Every check comes before any launch, in the header's order.
#include <math.h>

#include "corr_pyramid.h"

extern "C" int fn2y_abi_version(void) { return FN2Y_ABI_VERSION; }

namespace {
// checks 1 - 3 and 5 on what both entry points share; `ptrs` (the levels or their gradients) may be NULL until check 4, which the
// caller makes on its own pointers through `given`.  FN2_OK with p.B == 0 means "nothing to launch".
int make_params(fn2::PyramidP &p, const void *const *ptrs, bool entries_required, int num_levels, int B, int C, int H, int W, int H2, int W2,
                bool given, const void *a, const void *b)
{
    if (num_levels < 1 || num_levels > FN2Y_MAX_LEVELS) return FN2_EINVAL;
    if (B < 0 || C < 1 || H < 1 || W < 1 || H2 < 1 || W2 < 1) return FN2_EINVAL;
    if ((H2 >> (num_levels - 1)) == 0 || (W2 >> (num_levels - 1)) == 0) return FN2_EINVAL;
    const long long lim = 0x7fffffffLL, plane = (long long)H * W, slice = (long long)H2 * W2;
    if (plane > lim || B * plane > lim || slice > lim || C > (1 << 20)) return FN2_EUNSUPPORTED;   // (no product overflows 64 bits)
    if (B * plane * slice > (1LL << 48)) return FN2_EUNSUPPORTED;
    p = fn2::PyramidP{};
    p.L = num_levels;
    p.B = B;
    p.C = C;
    p.H = H;
    p.W = W;
    p.H2 = H2;
    p.W2 = W2;
    p.s = (float)(1.0 / sqrt((double)C));
    if (B == 0) return FN2_OK;
    if (!ptrs || !given) return FN2_EINVAL;
    if (entries_required)
        for (int l = 0; l < num_levels; ++l)
            if (!ptrs[l]) return FN2_EINVAL;
    if ((a && !fn2::aligned(a, 4)) || (b && !fn2::aligned(b, 4))) return FN2_EALIGN;
    for (int l = 0; l < num_levels; ++l) {
        if (!fn2::aligned(ptrs[l], 4)) return FN2_EALIGN;
        p.lvl[l] = static_cast<float *>(const_cast<void *>(ptrs[l]));
    }
    return FN2_OK;
}
} // namespace

extern "C" int fn2y_corr_pyramid_forward(const void *fmap1, const void *fmap2, void *const *levels, int num_levels, int B, int C, int H,
                                         int W, int H2, int W2, void *stream)
{
    fn2::PyramidP p;
    const int rc = make_params(p, levels, true, num_levels, B, C, H, W, H2, W2, fmap1 && fmap2, fmap1, fmap2);
    if (rc != FN2_OK || B == 0) return rc;
    return fn2::pyramid_forward(static_cast<const float *>(fmap1), static_cast<const float *>(fmap2), p, static_cast<hipStream_t>(stream));
}

extern "C" int fn2y_corr_pyramid_fold(const void *const *grad_levels, int num_levels, void *G, int B, int C, int H, int W, int H2, int W2,
                                      void *stream)
{
    fn2::PyramidP p;
    const int rc = make_params(p, grad_levels, false, num_levels, B, C, H, W, H2, W2, G != nullptr, G, nullptr);
    if (rc != FN2_OK || B == 0) return rc;
    return fn2::pyramid_fold(p, static_cast<float *>(G), static_cast<hipStream_t>(stream));
}
