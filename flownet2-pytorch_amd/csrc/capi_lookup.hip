// capi_lookup.hip -- C-ABI entry points of libflownet2_hip_lookup.so (include/flownet2_hip_lookup.h): CorrLookup.  Self-contained:
// links nothing of the other two libraries.  Every check comes before any launch.
#include "corr_lookup.h"   // (brings flownet2_hip.h: the codes and element types the lookup header restates)
#include "../../include/flownet2_hip_lookup.h"

extern "C" int fn2l_abi_version(void) { return FN2L_ABI_VERSION; }

namespace {
// AUTO -> the kernel it takes; FN2_OK, or the selector's rejection
int pick(int algo, const fn2::LookupP &p, bool &staged)
{
    if (algo < FN2L_LOOKUP_AUTO || algo > FN2L_LOOKUP_STAGED) return FN2_EINVAL;
    if (algo == FN2L_LOOKUP_STAGED && !fn2::lookup_staged_applicable(p)) return FN2_EUNSUPPORTED;
    staged = algo == FN2L_LOOKUP_STAGED || (algo == FN2L_LOOKUP_AUTO && fn2::lookup_staged_pays(p));
    return FN2_OK;
}
} // namespace

extern "C" int fn2l_corr_lookup_forward(const void *fmap1, const void *fmap2, const void *coords, void *out, int dtype, int B, int C,
                                        int H, int W, int H2, int W2, int radius, float scale, int algo, void *stream)
{
    using namespace fn2;
    if (dtype != FN2_F32) return FN2_EDTYPE;
    LookupP p;
    int rc = lookup_make_params(p, B, C, H, W, H2, W2, radius, scale);
    if (rc != FN2_OK) return rc;
    if (B == 0) return FN2_OK;
    if (!fmap1 || !fmap2 || !coords || !out) return FN2_EINVAL;
    if (!aligned(fmap1, 4) || !aligned(fmap2, 4) || !aligned(coords, 4) || !aligned(out, 4)) return FN2_EALIGN;
    bool staged = false;
    if ((rc = pick(algo, p, staged)) != FN2_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float *f1 = static_cast<const float *>(fmap1), *f2 = static_cast<const float *>(fmap2), *co = static_cast<const float *>(coords);
    return staged ? lookup_forward_staged(f1, f2, co, static_cast<float *>(out), p, s)
                  : lookup_forward_general(f1, f2, co, static_cast<float *>(out), p, s);
}

extern "C" int fn2l_corr_lookup_backward(const void *fmap1, const void *fmap2, const void *coords, const void *grad_out, void *grad_fmap1,
                                         void *grad_fmap2, int dtype, int B, int C, int H, int W, int H2, int W2, int radius, float scale,
                                         int algo, void *stream)
{
    using namespace fn2;
    if (dtype != FN2_F32) return FN2_EDTYPE;
    LookupP p;
    int rc = lookup_make_params(p, B, C, H, W, H2, W2, radius, scale);
    if (rc != FN2_OK) return rc;
    if (B == 0) return FN2_OK;
    if (!fmap1 || !fmap2 || !coords || !grad_out || !grad_fmap1 || !grad_fmap2) return FN2_EINVAL;
    if (!aligned(fmap1, 4) || !aligned(fmap2, 4) || !aligned(coords, 4) || !aligned(grad_out, 4) || !aligned(grad_fmap1, 4) ||
        !aligned(grad_fmap2, 4))
        return FN2_EALIGN;
    bool staged = false;
    if ((rc = pick(algo, p, staged)) != FN2_OK) return rc;
    return lookup_backward(static_cast<const float *>(fmap1), static_cast<const float *>(fmap2), static_cast<const float *>(coords),
                           static_cast<const float *>(grad_out), static_cast<float *>(grad_fmap1), static_cast<float *>(grad_fmap2), p,
                           staged, static_cast<hipStream_t>(stream));
}
