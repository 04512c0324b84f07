// binding_status.h -- the text a caller sees when the C ABI of a sibling library rejects a call (host C++, no torch: a
// stand-alone program can print it, tests/test_status_text_host.py).  fn2_strerror lives in libflownet2_hip.so, which the
// sibling modules do not link: the codes of each sibling header are spelled out here, once per library.
#pragma once
#include <string>

#include "flownet2_hip.h"

namespace fn2b {

// A library's tag and its wording for the four codes; nullptr where it has none (the code then reads "unknown error").
struct StatusText {
    const char *tag, *einval, *edtype, *ealign, *eunsupported;
};

constexpr StatusText STATUS_EXT = {"flownet2_hip_ext", "invalid shape or parameter", "dtype not supported by this op",
                                   "pointer not aligned to its element size",
                                   "unsupported parameter combination (the backward needs stride1 == 1)"};
constexpr StatusText STATUS_LOOKUP = {"flownet2_hip_lookup", "invalid shape or parameter (radius must be 0 .. 8)",
                                      "dtype not supported by this op (float32 only)", "pointer not aligned to its element size",
                                      "unsupported size or selector"};
constexpr StatusText STATUS_UPSAMPLE = {"flownet2_hip_upsample", "invalid shape or parameter (factor must be 2, 4 or 8)",
                                        "dtype not supported by this op (mask: float32, float16 or bfloat16)",
                                        "pointer not aligned to its element size", "unsupported size (at most 4 flow channels)"};
constexpr StatusText STATUS_SPLAT = {"flownet2_hip_splat", "invalid shape, selector or workspace", nullptr,
                                     "pointer not aligned to its element size",
                                     "unsupported size (a plane of 2^31 elements or more, or too many planes)"};
constexpr StatusText STATUS_CENSUS = {"flownet2_hip_census", "invalid shape or parameter", nullptr, "pointer not aligned to its element size",
                                      "unsupported size (a plane of 2^31 elements or more, or too many planes)"};
constexpr StatusText STATUS_SMOOTH = {"flownet2_hip_smooth", "invalid shape or parameter", nullptr, "pointer not aligned to its element size",
                                      "unsupported size (a plane of 2^31 elements or more, or too many planes)"};
// preview (include/preview/flownet2_hip_sample.h)
constexpr StatusText STATUS_SAMPLE = {"flownet2_hip_sample", "invalid shape or parameter (1 .. 8 levels, radius 0 .. 8)", nullptr,
                                      "pointer not aligned to its element size",
                                      "unsupported size (2^31 query pixels or more, a slice of 2^31 cells or more, or a level beyond 2^48 cells)"};
// incubating (include/preview/flownet2_hip_pyramid.h)
constexpr StatusText STATUS_PYRAMID = {"flownet2_hip_pyramid", "invalid shape, layout or parameter (contiguous maps, 1 .. 4 levels, none of them empty)",
                                       "dtype not supported by this op (float32 only: convert with .float())",
                                       "pointer not aligned to its element size",
                                       "unsupported size (2^31 query pixels or more, a slice of 2^31 cells or more, a volume beyond 2^48 cells, "
                                       "more than 2^20 channels, or 2^31 workgroups or more)"};
// staging (include/staging/flownet2_hip_ssim.h)
constexpr StatusText STATUS_SSIM = {"flownet2_hip_ssim",
                                    "invalid shape or parameter (max_distance 1 .. 3, c1 and c2 finite and > 0, border reflect needs H and W above "
                                    "max_distance)",
                                    nullptr, "pointer not aligned to its element size",
                                    "unsupported size (a plane of 2^31 elements or more, or too many planes)"};
// staging (include/staging/flownet2_hip_sample1d.h)
constexpr StatusText STATUS_SAMPLE1D = {"flownet2_hip_sample1d",
                                        "invalid shape or parameter (1 .. 8 levels, radius 0 .. 8, a coords batch stride of at least H W)", nullptr,
                                        "pointer not aligned to its element size",
                                        "unsupported size (2^31 query pixels or more, or a level beyond 2^48 cells)"};

// "<op>: HIP call failed: <tag>: <text> (code <rc>)" for rc != FN2_OK.  Failure path only: callers test rc first.
inline std::string status_message(const StatusText &lib, const char *op, int rc)
{
    const char *text = rc == FN2_EINVAL ? lib.einval : rc == FN2_EDTYPE ? lib.edtype : rc == FN2_EALIGN ? lib.ealign
                       : rc == FN2_EUNSUPPORTED ? lib.eunsupported : nullptr;
    if (!text) text = rc > 0 ? "hipError_t from the launch" : "unknown error";
    return std::string(op) + ": HIP call failed: " + lib.tag + ": " + text + " (code " + std::to_string(rc) + ")";
}

} // namespace fn2b
