// capi_census.hip -- C-ABI entry points of libflownet2_hip_census.so (include/flownet2_hip_census.h): the ternary census distance.
// Self-contained: links nothing of the other five libraries.  Every check comes before any launch, in the header's order.
#include "census.h"   // (brings flownet2_hip.h: the codes the census header restates)
#include "../../include/flownet2_hip_census.h"

extern "C" int fn2c_abi_version(void) { return FN2C_ABI_VERSION; }

extern "C" int fn2c_census_forward(const void *im1, const void *im2, void *out, int N, int C, int H, int W, int max_distance, float scale,
                                   int normalize, void *stream)
{
    using namespace fn2;
    CensusP p;
    int rc = census_make_params(p, N, C, H, W);
    if (rc != FN2_OK) return rc;
    if (N == 0) return FN2_OK;
    if (!im1 || !im2 || !out) return FN2_EINVAL;
    if (!aligned(im1, 4) || !aligned(im2, 4) || !aligned(out, 4)) return FN2_EALIGN;
    if ((rc = census_set_options(p, max_distance, scale, normalize)) != FN2_OK) return rc;
    return census_forward(static_cast<const float *>(im1), static_cast<const float *>(im2), static_cast<float *>(out), p,
                          static_cast<hipStream_t>(stream));
}

extern "C" int fn2c_census_backward(const void *im1, const void *im2, const void *grad_out, void *grad_im1, void *grad_im2, int N, int C,
                                    int H, int W, int max_distance, float scale, int normalize, void *stream)
{
    using namespace fn2;
    CensusP p;
    int rc = census_make_params(p, N, C, H, W);
    if (rc != FN2_OK) return rc;
    if (N == 0) return FN2_OK;
    if (!im1 || !im2 || !grad_out || (!grad_im1 && !grad_im2)) return FN2_EINVAL;
    if (!aligned(im1, 4) || !aligned(im2, 4) || !aligned(grad_out, 4) || !aligned(grad_im1, 4) || !aligned(grad_im2, 4)) return FN2_EALIGN;
    if ((rc = census_set_options(p, max_distance, scale, normalize)) != FN2_OK) return rc;
    return census_backward(static_cast<const float *>(im1), static_cast<const float *>(im2), static_cast<const float *>(grad_out),
                           static_cast<float *>(grad_im1), static_cast<float *>(grad_im2), p, static_cast<hipStream_t>(stream));
}
