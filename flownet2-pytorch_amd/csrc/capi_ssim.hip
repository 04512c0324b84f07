// capi_ssim.hip -- C-ABI entry points of libflownet2_hip_ssim.so (include/staging/flownet2_hip_ssim.h): the structural-similarity
// distance.  Self-contained: links nothing of the other libraries.  Every check comes before any launch, in the header's order.
#include "ssim.h"   // (brings flownet2_hip.h: the codes the staging header restates)
#include "../../include/staging/flownet2_hip_ssim.h"

extern "C" int fn2i_abi_version(void) { return FN2I_ABI_VERSION; }

extern "C" int fn2i_ssim_forward(const void *im1, const void *im2, void *out, int N, int C, int H, int W, int md, float c1, float c2,
                                 int border, void *stream)
{
    using namespace fn2;
    SsimP p;
    int rc = ssim_make_params(p, N, C, H, W);
    if (rc != FN2_OK) return rc;
    if ((rc = ssim_set_options(p, md, c1, c2, border)) != FN2_OK) return rc;
    if (N == 0) return FN2_OK;
    if (!im1 || !im2 || !out) return FN2_EINVAL;
    if (!aligned(im1, 4) || !aligned(im2, 4) || !aligned(out, 4)) return FN2_EALIGN;
    return ssim_forward(static_cast<const float *>(im1), static_cast<const float *>(im2), static_cast<float *>(out), p,
                        static_cast<hipStream_t>(stream));
}

extern "C" int fn2i_ssim_backward(const void *im1, const void *im2, const void *grad_out, void *grad1, void *grad2, int N, int C, int H,
                                  int W, int md, float c1, float c2, int border, void *stream)
{
    using namespace fn2;
    SsimP p;
    int rc = ssim_make_params(p, N, C, H, W);
    if (rc != FN2_OK) return rc;
    if ((rc = ssim_set_options(p, md, c1, c2, border)) != FN2_OK) return rc;
    if (N == 0) return FN2_OK;
    if (!im1 || !im2 || !grad_out || (!grad1 && !grad2)) return FN2_EINVAL;
    if (!aligned(im1, 4) || !aligned(im2, 4) || !aligned(grad_out, 4) || !aligned(grad1, 4) || !aligned(grad2, 4)) return FN2_EALIGN;
    return ssim_backward(static_cast<const float *>(im1), static_cast<const float *>(im2), static_cast<const float *>(grad_out),
                         static_cast<float *>(grad1), static_cast<float *>(grad2), p, static_cast<hipStream_t>(stream));
}
