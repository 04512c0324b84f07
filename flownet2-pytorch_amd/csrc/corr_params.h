// corr_params.h -- correlation parameter block shared by the dispatcher and the kernel files.
#pragma once
#include "fn2_common.h"

namespace fn2 {

struct CorrP {
    int B, C, H, W;            // input1 / input2 shape (NCHW)
    int pad, k, md, s1, s2;    // pad_size, kernel_size, max_displacement, stride1, stride2
    int kr, dr, D, nOut, oH, oW;
    long out_bs;               // elements between batch items of the output (nOut*oH*oW unless it is a slice of a larger buffer)
    float slope;               // LeakyReLU negative slope applied to the output (1 = none)
};

// One correlation call as the dispatcher (capi.hip) hands it to a launcher: the tensors of its direction (forward: in1, in2, out;
// backward: in1, in2, gout, g1, g2) and the launcher's own tune / variant value (0 = the product kernel)
struct CorrCall {
    int dtype;
    CorrP p;
    const void *in1, *in2, *gout;
    void *out, *g1, *g2;
    int tune;
};
typedef bool CorrPredicate(int dtype, const CorrP &p);        // a kernel's domain: pure, no pointer is looked at
typedef int CorrLauncher(const CorrCall &c, hipStream_t s);   // FN2_EUNSUPPORTED / FN2_EALIGN: declined, nothing launched

int corr_make_params(CorrP &p, int B, int C, int H, int W, int pad, int k, int md, int s1, int s2);
int corr_dispatch(int direction, CorrCall &c, int algo, bool debug_variant, hipStream_t s);   // capi.hip; direction 0 forward, 1 backward
CorrLauncher corr_forward_direct, corr_backward_direct;

// dense stride-1 cost volumes (PWC-Net: k = 1, s1 = s2 = 1, pad == md, 1 <= md <= 4; f32 / f16 / bf16; correlation_dense.hip): LDS-tiled
// VALU kernels with the bits of corr_*_direct.  They decline (FN2_EUNSUPPORTED, nothing launched) outside that domain and for
// shapes beyond their 32-bit offsets; p.out_bs and p.slope are honoured like in corr_forward_direct
CorrPredicate corr_dense_applicable;
bool corr_dense_forward_pays(const CorrP &p);   // enough workgroups for the dense forward to beat the general kernel (AUTO asks; the debug variant does not)
CorrLauncher corr_forward_dense, corr_backward_dense;

// float tensors on the fp32 matrix cores (correlation_mfma.hip, correlation_mfma_bwd.hip); c.tune: see the launchers
CorrPredicate corr_mfma_f32_applicable, corr_bwd_mfma_f32_applicable;
CorrLauncher corr_forward_mfma_f32, corr_backward_mfma_f32;

// float tensors, two-term f16 split (correlation_f16x2*.hip); c.tune: the profiling variant.  _wide: W > 64, called by the other two
CorrPredicate corr_f16x2_applicable, corr_bwd_f16x2_applicable;
CorrLauncher corr_forward_f16x2, corr_forward_f16x2_wide, corr_backward_f16x2, corr_backward_f16x2_wide;
void corr_f16x2_set_debug_buffer(void *p);
void *corr_f16x2_get_debug_buffer();

// half and bfloat16 tensors (correlation_f16_fwd.hip, correlation_f16_bwd.hip): one 16-bit MFMA per block product, no split, fp32 sums
CorrPredicate corr_f16_fwd_applicable, corr_f16_bwd_applicable;
CorrLauncher corr_forward_f16, corr_backward_f16;

// double tensors on the fp64 matrix cores (correlation_mfma_f64.hip): FlowNetC's configuration, md = 20
CorrPredicate corr_mfma_f64_applicable;
CorrLauncher corr_forward_mfma_f64, corr_backward_mfma_f64;

// Neighbour row blocks of a backward task (FlowNetC's configuration: 4 centre lattice rows per row group rg, displacement radius dr
// lattice rows, nu = ceil((2 dr + 4) / 4) blocks of 4 neighbour rows: block u holds lattice rows 4rg - dr + 4u .. +3 of a parity
// lattice of HL rows).  A block is REAL iff one of its rows lies in [0, HL): 4rg - dr + 4u + 3 >= 0 and 4rg - dr + 4u <= HL - 1 (the
// rule of correlation_mfma_bwd.hip); a block that is not contributes zeros only (its X rows do not exist) and is not walked.  The
// range is never empty for a row group of the image (4rg <= HL - 1): the blocks that hold the centre rows themselves meet it.
struct URange { int lo, hi; };
__host__ __device__ constexpr URange bwd_u_range(int rg, int HL, int dr = 10, int nu = 6)
{
    const int lo = (dr - 4 * rg) >> 2, hi = (HL - 1 + dr - 4 * rg) >> 2;   // ceil((dr - 3 - 4rg) / 4), floor((HL - 1 + dr - 4rg) / 4)
    return URange{lo < 0 ? 0 : lo, hi > nu - 1 ? nu - 1 : hi};
}
static_assert(bwd_u_range(0, 24).lo == 2 && bwd_u_range(1, 24).lo == 1 && bwd_u_range(2, 24).lo == 0 && bwd_u_range(3, 24).hi == 5 &&
              bwd_u_range(4, 24).hi == 4 && bwd_u_range(5, 24).hi == 3 && bwd_u_range(0, 1).lo == 2 && bwd_u_range(0, 1).hi == 2, "real row blocks");

} // namespace fn2
