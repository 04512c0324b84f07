"""Per-element error bounds of the float32 and float64 correlation kernels -- TEST INFRASTRUCTURE ONLY.

One bound (delta) per documented contract of include/flownet2_hip.h, in float64 per output element; the kernel's output must
lie in lowp_ref.bracket(ref64, delta, torch.float32): ref64 +- delta rounded outward to fp32 (with the fused LeakyReLU applied
to both ends as a monotone post step).  The references are lowp_ref.corr_fwd64 / corr_bwd64 (torch float64, on the device the
tensors are on).  Every bound scales with the element's own sum of |terms| (abs_ref), never with the largest output.

Units: U23 = 2^-23 is the fp32 rounding unit doubled (lowp_ref: the bounds hold if the matrix cores' sums truncate).

The f16x2 kernels (FN2_CORR_MFMA_F16X2) need m, the typical magnitude each operand's scale places at 2^-1: m = 2^(e - 127) with
e the rounded mean biased exponent of the sample's non-zero values (f16x2_split.h scale_exp), hence m <= the largest |x| the
sample can read.  The helpers below bound m from above by the largest |x| over every element that the task's sample can read
(derived from the sample code, see each helper); where that region holds a zero or an fp32 subnormal (exponent field 0: not
counted by exp_stat) the sample might see nothing and leave the operand unscaled, m = 2^-1 (lowp_ref's convention).
"""
import torch

import lowp_ref as L

U23 = L.U23
U52 = 2.0 ** -52
F32_SUB = 2.0 ** -149     # one fp32 subnormal step: the absolute error of one rounding into the subnormal range (doubled)
TINY = 2.0 ** -126        # below this exp_stat sees a zero exponent field
M_CAP = 2.0 ** 125        # the largest m: scale_exp clamps k to >= -126 (a sample of inf / nan included)


# ------------------------------------------------------------------ the typical magnitudes m (upper bounds)
def _region_max(ax, y_lo, y_hi, x_lo=None, x_hi=None):
    """max over rows [y_lo, y_hi) (clipped to the image), columns [x_lo, x_hi) and dims 1.. of ax (B, ..., H, W); a region
    that holds a zero or subnormal, or no element at all, gives at least 2^-1."""
    H, W = ax.shape[-2:]
    y_lo, y_hi = max(0, y_lo), min(H, y_hi)
    x_lo, x_hi = max(0, 0 if x_lo is None else x_lo), min(W, W if x_hi is None else x_hi)
    B = ax.shape[0]
    if y_lo >= y_hi or x_lo >= x_hi:
        return torch.full((B,), 0.5, dtype=torch.float64, device=ax.device)
    r = ax[..., y_lo:y_hi, x_lo:x_hi].reshape(B, -1)
    m = r.nan_to_num(nan=M_CAP, posinf=M_CAP).amax(1).clamp(max=M_CAP)
    return torch.where((r < TINY).any(1), m.clamp(min=0.5), m)


def m_fwd_narrow(a, b):
    """(mA, mB) of the narrow f16x2 forward (correlation_f16x2.hip sample_issue), as (B, 1, H, W) float64 tensors; mA at the in1
    pixel, mB at the in2 pixel.  A task (n, py, rg, u) samples in1 lattice rows 4 rg .. 4 rg + 3 of parity py (image rows
    8 rg .. 8 rg + 7, taken here for both parities), 64 channels and 16 columns of the whole width: bounded by those image rows,
    every channel and column.  Its B sample reads in2 lattice rows 4 rg - 10 + 4 u .. + 3, i.e. the aligned group 4 q + 2 .. 4 q + 5
    that holds the B pixel's lattice row: image rows 8 q + 4 .. 8 q + 11."""
    B, C, H, W = a.shape
    aa, ab = a.double().abs(), b.double().abs()
    mA = torch.empty(B, 1, H, W, dtype=torch.float64, device=a.device)
    mB = torch.empty_like(mA)
    for y0 in range(0, H, 8):
        mA[:, 0, y0:y0 + 8] = _region_max(aa, y0, y0 + 8)[:, None, None]
    for y0 in range(-4, H, 8):
        mB[:, 0, max(0, y0):y0 + 8] = _region_max(ab, y0, y0 + 8)[:, None, None]
    return mA, mB


def m_fwd_wide(a, b, wpx=32):
    """(mA, mB) of the column-window f16x2 forward (correlation_f16x2_wide.hip sample_issue).  A task takes two row groups rg0,
    rg0 + 1 and one 32-pixel window xq; its A sample reads one of the two row groups (rga) inside the window, and the scale is
    applied to both: mA at an in1 pixel of row group rg is bounded by rows of row groups rg - 1 .. rg + 1 (whichever pairing)
    inside the pixel's window.  The B sample reads the B row block (aligned group 4 q + 2 .. 4 q + 5, as the narrow kernel) in
    columns 32 xq - 16 .. 32 xq + 47; the windows whose pixels reach an in2 pixel x_b (|x - x_b| <= 20) sample inside
    x_b - 67 .. x_b + 67: mB is bounded by that span of the B pixel's row block."""
    B, C, H, W = a.shape
    aa, ab = a.double().abs(), b.double().abs()
    mA = torch.empty(B, 1, H, W, dtype=torch.float64, device=a.device)
    mB = torch.empty_like(mA)
    for y0 in range(0, H, 8):
        for x0 in range(0, W, wpx):
            mA[:, 0, y0:y0 + 8, x0:x0 + wpx] = _region_max(aa, y0 - 8, y0 + 16, x0, x0 + wpx)[:, None, None]
    for y0 in range(-4, H, 8):
        lo, hi = max(0, y0), min(H, y0 + 8)
        if lo >= hi:
            continue
        r = ab[:, :, lo:hi].transpose(1, 3).reshape(B, W, -1)          # (B, column, values)
        cmax = torch.nn.functional.max_pool1d(r.nan_to_num(nan=M_CAP, posinf=M_CAP).amax(2)[:, None], 135, 1, 67)[:, 0].clamp(max=M_CAP)
        czero = torch.nn.functional.max_pool1d((r < TINY).any(2).double()[:, None], 135, 1, 67)[:, 0] > 0
        mB[:, 0, lo:hi] = torch.where(czero, cmax.clamp(min=0.5), cmax)[:, None, :]
    return mA, mB


def m_bwd_x(x):
    """Per-channel magnitude of the backward's X operand (correlation_f16x2_bwd*.hip sample_issue), (B, C, H, W): a task of row
    group rg samples each channel at lattice rows 4 rg .. 4 rg + 3 (clamped into the image) of its parity -- image rows
    8 rg .. 8 rg + 7 -- and applies the scale to every value of that channel it reads; bounded by the channel's largest |value|
    in those rows, whole width (the wide kernel samples inside its 64-pixel window: a subset), at the gradient element's row."""
    ax = x.double().abs().nan_to_num(nan=M_CAP, posinf=M_CAP).clamp(max=M_CAP)
    m = torch.empty_like(ax)
    H = x.shape[2]
    for y0 in range(0, H, 8):
        blk = ax[:, :, y0:y0 + 8]
        bm = blk.amax(dim=(2, 3), keepdim=True)
        bm = torch.where((blk < TINY).flatten(2).any(2)[..., None, None], bm.clamp(min=0.5), bm)
        m[:, :, y0:y0 + 8] = bm
    return m


def m_bwd_g(go, H, W):
    """gradOutput magnitude of a backward task, (B, 1, H, W) at the gradient element's row: the G sample reads displacement
    rows tj = 8 + bi - ai (grad_in1 tasks) or 12 - bi + ai (grad_in2 tasks) -- 5 .. 15 --, any displacement column, lattice rows
    4 rg .. 4 rg + 3 (grad_in1) or 4 rg - 2 .. 4 rg + 1 (grad_in2) of the task's parity: image rows 8 rg - 4 .. 8 rg + 7, whole
    width.  One scale per task."""
    B = go.shape[0]
    D = 21
    g = go.double().abs().view(B, D, D, H, W)[:, 5:16]
    m = torch.empty(B, 1, H, W, dtype=torch.float64, device=go.device)
    for y0 in range(0, H, 8):
        m[:, 0, y0:y0 + 8] = _region_max(g, y0 - 4, y0 + 8)[:, None, None]
    return m


# ------------------------------------------------------------------ per-term error of the two-term split
# An operand x with scale 2^k (m = 2^-k / 2) is held as h + l: |x - (h + l) 2^-k| <= e(x) = max(2^-22 |x|, 2^-24 m) (the 2^-24 m
# floor: half of the smallest f16 subnormal step, 2^-25, in scaled units where m sits at 2^-1), |l| 2^-k <= 2^-11 |x| + 2^-24 m.
# The kernel forms ah bh + ah bl + al bh exactly (11 x 11 bit products fit fp32) and drops al bl.  Per product a b:
#   |error| <= e(a) |b| + |a| e(b) + e(a) e(b) + |al bl|
#           <= (2^-21 + 2^-22 + 2^-44) |a b| + (2^-24 + 2^-35 + 2^-46) (m_a |b| + m_b |a|) + 2^-47 m_a m_b
C_REL = 2.0 ** -21 + 2.0 ** -22 + 2.0 ** -44
C_FLOOR = 2.0 ** -24 + 2.0 ** -35 + 2.0 ** -46
C_MM = 2.0 ** -47


def delta_f16x2_fwd(ref, absr, s_mb_a, s_ma_b, s_mm, C):
    """FN2_CORR_MFMA_F16X2 forward, narrow and column-window (correlation_f16x2*.hip).  Per output (all sums already / C, as
    corr_fwd64 forms them): the split terms above over the element's C products (s_mb_a = sum_c m_B |a| / C, s_ma_b = sum_c
    m_A |b| / C, s_mm = sum_c m_A m_B / C); then fp32 sums of 3 C partial products (each |partial| <= (1 + 2^-9) |a b| plus the
    floor terms); then the epilogue: v_ldexp_f32 by -(ka + kb) - log2 C for a power-of-two C (exact unless the result is an fp32
    subnormal), for any other C ldexp by -(ka + kb) and an IEEE division by C (correlation_f16x2.hip store_rows): one more
    rounding, U23 |ref|, and an absolute floor of two subnormal steps where the result lies in the fp32 subnormal range (the
    header is silent on subnormal outputs; this assumes they are kept, as fp32 arithmetic does with denormals enabled)."""
    pow2 = (C & (C - 1)) == 0
    split = C_REL * absr + C_FLOOR * (s_mb_a + s_ma_b) + C_MM * s_mm
    sums = 3 * C * U23 * ((1 + 2.0 ** -9) * absr + C_FLOOR * (s_mb_a + s_ma_b))
    epi = (0.0 if pow2 else U23) * ref.abs() + (1 if pow2 else 2) * F32_SUB
    return split + sums + epi


def delta_f16x2_bwd(ref, absr, s_mx_g, s_mg_x, s_mm, n):
    """FN2_CORR_MFMA_F16X2 backward, narrow and column-window: X (in2 for grad_in1, in1 for grad_in2) has one scale per channel
    and task, G (gradOutput) one per task; the split terms over the element's n = 441 (displacement) products, fp32 sums of 3 n
    partial products, the 1/C step (multiply by the exact 2^-log2 C or divide: U23 |ref|) and the subnormal floor."""
    split = C_REL * absr + C_FLOOR * (s_mx_g + s_mg_x) + C_MM * s_mm
    sums = 3 * n * U23 * ((1 + 2.0 ** -9) * absr + C_FLOOR * (s_mx_g + s_mg_x))
    return split + sums + U23 * ref.abs() + 2 * F32_SUB


def delta_bf16x3(ref, absr, n, C=None):
    """FN2_CORR_MFMA_BF16X3: x = h + m + l in bf16, exact (8 + 8 + 8 significant bits), |m| <= 2^-8 |x|, |l| <= 2^-16 |x|; the
    kernel keeps hh, hm, mh, hl, lh, mm and drops ml, lm, ll: <= (2 * 2^-24 + 2^-32) |a b| per product.  fp32 sums of 6 n partial
    products (n = C forward, 441 backward, over C), the 1/C step, one subnormal step per rounding.  Holds for operands in fp32's normal range above
    2^-110 (the split's smallest term stays normal)."""
    C = n if C is None else C
    return (2 * 2.0 ** -24 + 2.0 ** -32) * absr + 6 * n * U23 * (1 + 2.0 ** -7) * absr + U23 * ref.abs() + \
        (6 * n + 1) * F32_SUB / C + F32_SUB


def delta_fma_chain(ref, absr, n, C=None):
    """FN2_CORR_MFMA_F32 ("bitwise an fmaf chain") and the f16x2 kernels' out-of-range recompute (exact_corr / exact_grad): a
    chain of n fused multiply-adds rounds once per step, |error| <= n U23 sum |a b|; then the 1/C step (U23 |ref|).  Where the
    terms or the result are fp32 subnormals each of the n + 1 roundings adds up to one subnormal step: (n + 1) 2^-149 on the sum,
    divided by C (C = n in the forward; 441 terms over C in the backward), plus one for the final rounding."""
    C = n if C is None else C
    return n * U23 * absr + U23 * ref.abs() + (n + 1) * F32_SUB / C + F32_SUB


def delta_direct_f32(ref, absr, C, k=1):
    """FN2_CORR_DIRECT forward, float32 and float64 tensors (correlation_direct.hip corr_fwd_direct; the double kernel
    accumulates in float, as the reference's float accumulator does -- tests/test_correlation_f64.py): every product rounded
    to fp32; four interleaved partial sums, s1 .. s3 of floor(C / 4) terms and s0 of floor(C / 4) + C % 4 (the leftover
    channels go to s0); two pairwise adds; one add per window pixel (k^2); acc / (k^2 C) rounded:
    (1 + floor(C/4) + C % 4 + 2 + k^2) U23 relative to abs_ref, U23 |ref|, and one subnormal step per rounding."""
    depth = 1 + C // 4 + C % 4 + 2 + k * k
    nel = k * k * C
    return depth * U23 * absr + U23 * ref.abs() + (nel + depth + 1) * F32_SUB / nel + F32_SUB


def delta_direct_bwd_f32(ref, absr, n_terms):
    """FN2_CORR_DIRECT backward, float32 (correlation_direct.hip corr_bwd_direct): per displacement the window's gradOutput
    summed (k^2 - 1 adds), times the other input (one rounding), added to a sequential fp32 sum over the D^2 displacements;
    n_terms = D^2 k^2 >= that depth; / (k^2 C) rounded."""
    return (n_terms + 1) * U23 * absr + U23 * ref.abs() + 2 * F32_SUB


def delta_direct_bwd_f64(ref, absr, n_terms):
    """FN2_CORR_DIRECT backward, double tensors: the same sums, accumulated in double (Acc<double>)."""
    return delta_f64(ref, absr, n_terms)


def delta_f64(ref, absr, n):
    """fp64 MFMA kernel (correlation_mfma_f64.hip, v_mfma_f64_16x16x4_f64): products and sums in fp64, / C in fp64."""
    return (n + 1) * U52 * absr + U52 * ref.abs() + 2.0 ** -1070


def fwd_nonfinite(a, b, params):
    """Outputs that have a term whose two operands both lie in the image and whose product is not finite: where the kernels'
    outputs are inf / nan.  A read outside the image is an absent term, not a zero factor: inf next to the padding does not
    make the outputs that only pair it with the padding nan (the reference's 0 * inf would)."""
    one = torch.ones_like(a, dtype=torch.float64)
    na = (~torch.isfinite(a)).double().amax(1, keepdim=True).expand_as(one).contiguous()
    nb = (~torch.isfinite(b)).double().amax(1, keepdim=True).expand_as(one).contiguous()
    return (L.corr_fwd64(na, one, *params) + L.corr_fwd64(one, nb, *params)) > 0


def bwd_nonfinite(a, b, go, params):
    """(grad_in1, grad_in2) elements with a term whose gradOutput and in-image operand give a non-finite product (the backward
    skips terms outside the image, exact_grad and the general kernel alike)."""
    one = torch.ones_like(a, dtype=torch.float64)
    og = torch.ones_like(go, dtype=torch.float64)
    ng = (~torch.isfinite(go)).double()
    n1, _ = L.corr_bwd64(one, (~torch.isfinite(b)).double(), og, *params)
    _, n2 = L.corr_bwd64((~torch.isfinite(a)).double(), one, og, *params)
    g1, g2 = L.corr_bwd64(one, one, ng, *params)
    return (n1 + g1) > 0, (n2 + g2) > 0


def bwd_touched(a, b, go, params, thresh=65520.0):
    """(grad_in1, grad_in2) elements with a term whose in1 / in2 operand is at or above thresh (or not finite)."""
    one = torch.ones_like(a, dtype=torch.float64)
    og = torch.ones_like(go, dtype=torch.float64)
    t1, _ = L.corr_bwd64(one, (~(b.abs() < thresh)).double(), og, *params)
    _, t2 = L.corr_bwd64((~(a.abs() < thresh)).double(), one, og, *params)
    return t1 > 0, t2 > 0


def finite_part(x):
    """x with inf / nan replaced by 0: the float64 reference of every output fwd_nonfinite leaves finite."""
    return torch.where(torch.isfinite(x), x, torch.zeros_like(x))


# ------------------------------------------------------------------ per-element sums that the f16x2 bounds need
def fwd_sums(a, b, params, wide):
    """(ref, absr, s_mb_a, s_ma_b, s_mm) of the f16x2 forward, float64 (B, 441, oH, oW): the magnitudes from the operands as
    they are (a sample may read an inf / nan: m <= M_CAP), the sums from their finite parts (fwd_nonfinite names the rest)."""
    mA, mB = (m_fwd_wide if wide else m_fwd_narrow)(a, b)
    a, b = finite_part(a.double()), finite_part(b.double())
    ref = L.corr_fwd64(a, b, *params)
    absr = L.corr_fwd64(a.abs(), b.abs(), *params)
    ones = torch.ones_like(a, dtype=torch.float64)
    s_mb_a = L.corr_fwd64(a.abs(), mB.expand_as(ones), *params)
    s_ma_b = L.corr_fwd64(mA.expand_as(ones), b.abs(), *params)
    s_mm = L.corr_fwd64(mA.expand_as(ones), mB.expand_as(ones), *params)
    return ref, absr, s_mb_a, s_ma_b, s_mm


def bwd_deltas(a, b, go, params):
    """((r1, d1), (r2, d2)) of the f16x2 backward: grad_in1 = sum_d gO * in2 (X = in2), grad_in2 = sum_d gO * in1 (X = in1).
    Magnitudes from the operands as they are, sums from their finite parts (bwd_nonfinite names the rest).  Elements with a term
    at or above 65520 take the larger of this bound and the fp32 chain's: the recompute (exact_grad) runs where the scaled
    operand overflowed the f16, which depends on the channel's sample."""
    B, C, H, W = a.shape
    t1, t2 = bwd_touched(a, b, go, params)
    mx1, mx2 = m_bwd_x(b), m_bwd_x(a)                             # X of grad_in1 / grad_in2, at the gradient element's row
    a, b = finite_part(a.double()), finite_part(b.double())
    r1, r2 = L.corr_bwd64(a, b, go, *params)
    ab1, ab2 = L.corr_bwd64(a.abs(), b.abs(), go.abs(), *params)
    mg = m_bwd_g(go, H, W)                                        # at the gradient element's row
    ga = go.double().abs()
    ones_x = torch.ones_like(a, dtype=torch.float64)
    ones_g = torch.ones_like(ga)
    sg1, sg2 = L.corr_bwd64(ones_x, ones_x, ga, *params)           # sum |gO| over each element's terms (/ C)
    sb1, _ = L.corr_bwd64(ones_x, b.double().abs(), ones_g, *params)
    _, sa2 = L.corr_bwd64(a.double().abs(), ones_x, ones_g, *params)
    cnt1, cnt2 = L.corr_bwd64(ones_x, ones_x, ones_g, *params)      # number of terms (/ C)
    n = L.n_bwd(params[2], params[4], params[1])
    d1 = delta_f16x2_bwd(r1, ab1, mx1 * sg1, mg * sb1, mx1 * mg * cnt1, n)
    d2 = delta_f16x2_bwd(r2, ab2, mx2 * sg2, mg * sa2, mx2 * mg * cnt2, n)
    d1 = torch.where(t1, torch.maximum(d1, delta_fma_chain(r1, ab1, n, C)), d1)
    d2 = torch.where(t2, torch.maximum(d2, delta_fma_chain(r2, ab2, n, C)), d2)
    return (r1, d1), (r2, d2), (ab1, ab2)


# ------------------------------------------------------------------ input families with full 24-bit fp32 mantissas
FAMILIES = tuple(range(1, 11))


def _fill_mantissa(x, rng):
    """x (float64 numpy) with random low mantissa bits: no value is half- or bfloat16-representable."""
    import numpy as np
    f = x.astype(np.float32)
    bits = f.view(np.uint32) | (rng.integers(1, 1 << 13, f.shape, dtype=np.uint32) & 0x1FFF) | 1
    keep = (f != 0) & np.isfinite(f)
    return np.where(keep, bits.view(np.float32), f)


def family_inputs(family, shape, seed):
    """in1, in2 (CPU float32) of input family 1..10:
      1-5 lowp_ref.family_inputs with fp32 ranges: 2 per-channel 2^+-20, 5 row ramp 2^+-12;
      6 batch items at 2^+30, 2^-30, 1, 2^+30, ... (operands of each item; B >= 9 crosses the forward's persistent workgroups' items -- the
        backward's workgroups run a second task only past 256 tasks: test_gpu_f32_contract.BWD_MULTI);
      7 a ramp along the columns over 2^+-12 (the wide kernels' 32-pixel windows each see another magnitude);
      8 item 0 at 2^-66 (outputs in the fp32 subnormal range), the others at 2^+30 (outputs near 2^+60);
      9 normal data with scattered operands 65520, 1e6, -3e5, 2^20, ... (at or above 2^17 m for m <= 1/2: h overflows the f16,
        the outputs they touch are recomputed by the fp32 chain; finite products and sums stay finite), +inf in in1 at the
        top-left corner, nan in in2 at the bottom-right corner and, from 16 rows on, nan in in1 at the last row's middle: edge
        pixels, whose displacements reach the zero padding;
      10 every value the narrow forward's operand samples read is zero (correlation_f16x2.hip sample_issue: lane l reads channel
        l C / 64, lattice row 4 rg + (l & 3) -- in2: 4 rg + 2 + (l & 3) mod 4 --, 4 pixels from column 4 ((5 l / 4 mod 16) W / 4
        / 16)), so every task of that kernel leaves its operands unscaled; the rest at 1e-3 (h keeps 11 bits, l is an f16
        subnormal).  For the other kernels: scattered zeros in small data.
    Every finite non-zero value carries a full 24-bit mantissa."""
    import numpy as np
    B, C, H, W = shape
    rng = np.random.default_rng(seed * 10 + family)
    if family <= 5:
        a, b = (t.double().numpy() for t in L.family_inputs(family, shape, torch.bfloat16 if family in (2, 5) else torch.float32,
                                                            seed))
        if family in (2, 5):   # the bf16 ranges of lowp_ref, regenerated at full precision
            a0 = rng.standard_normal(shape)
            b0 = rng.standard_normal(shape)
            if family == 2:
                a = a0 * 2.0 ** rng.uniform(-20, 20, (1, C, 1, 1))
                b = b0 * 2.0 ** rng.uniform(-20, 20, (1, C, 1, 1))
            else:
                r = 2.0 ** (12.0 * (2.0 * np.arange(H) / max(H - 1, 1) - 1.0))
                a, b = a0 * r[None, None, :, None], b0 * r[None, None, :, None]
    else:
        a = rng.standard_normal(shape)
        b = rng.standard_normal(shape)
        if family == 6:
            s = np.array([2.0 ** 30, 2.0 ** -30, 1.0])[np.arange(B) % 3]
            a, b = a * s[:, None, None, None], b * s[:, None, None, None]
        elif family == 7:
            r = 2.0 ** (12.0 * (2.0 * np.arange(W) / max(W - 1, 1) - 1.0))
            a, b = a * r[None, None, None, :], b * r[None, None, None, :]
        elif family == 8:
            s = np.where(np.arange(B) == 0, 2.0 ** -66, 2.0 ** 30)
            a, b = a * s[:, None, None, None], b * s[:, None, None, None]
        elif family == 9:
            for t, vals in ((a, (65520.0, 1e6, -3e5, 2.0 ** 20)), (b, (65520.0, -1e6, 2.5e5, -2.0 ** 19))):
                idx = rng.choice(t.size, size=min(t.size, 6), replace=False)
                t.flat[idx] = np.array(vals * 2)[:idx.size]
            a[B - 1, rng.integers(C), 0, 0] = np.inf
            b[0, rng.integers(C), H - 1, W - 1] = np.nan
            if H >= 16:
                a[0, rng.integers(C), H - 1, W // 2] = np.nan
        elif family == 10:
            a, b = a * 1e-3, b * 1e-3
            lrow = (np.arange(H) >> 1) & 3                   # lattice row mod 4 of every image row
            for ln in range(64):
                c, x = (ln * C) >> 6, 4 * (((((5 * ln) >> 2) & 15) * (W >> 2)) >> 4)
                a[:, c, lrow == (ln & 3), x:x + 4] = 0.0
                b[:, c, lrow == ((ln + 2) & 3), x:x + 4] = 0.0
        else:
            raise AssertionError(family)
    a = _fill_mantissa(np.asarray(a), rng)
    b = _fill_mantissa(np.asarray(b), rng) if family != 4 else a * np.sign(np.asarray(b) * np.asarray(a) + 0.0).astype(np.float32)
    return torch.from_numpy(a), torch.from_numpy(b)


def grad_output(kind, shape, seed):
    """gradOutput (CPU float32): lowp_ref's 'normal', 'leaky', 'window'; 'planes' -- some displacement planes x 1e5; 'train' --
    the ~1e-7 scale of a training gradient; 'items' -- normal data, item n times (2^-40, 2^20, 1)[(n + 1) % 3]: offset against
    family 6's cycle (2^30, 2^-30, 1)[n % 3], so that along a batch the X and the G exponents of a backward task do not move
    together, and a persistent workgroup's next task (another item) has other scale exponents for both operands.  For B = 1 the
    rows [0, H/2) are times 2^-40 and the rows [H/2, H) times 2^20: the tasks of one item then differ by their row group.
    m_bwd_g takes its maximum per item and row band (the rows one task's G sample can read), so the bound's derivation is
    unchanged by this kind.  (B = 1: a grad_in2 task whose sample lies in the small rows reads gradOutput up to 10 lattice rows
    away, in the large ones; under its scale those values overflow the f16, the sums are not finite and the elements are
    recomputed by the fp32 chain (exact_grad), whose n U23 abs_ref + U23 |ref| lies inside delta_f16x2_bwd's 3 n U23 abs_ref
    + U23 |ref| -- these gradients are far above the fp32 subnormal range.  The other way round, small values under a large
    scale vanish within the 2^-24 m floor.)  Full 24-bit mantissas."""
    import numpy as np
    rng = np.random.default_rng(seed + 7)
    if kind in ("normal", "leaky", "window"):
        g = L.grad_output(kind, shape, torch.float32, seed).double().numpy()
    else:
        g = rng.standard_normal(shape)
        if kind == "planes":
            g[:, rng.choice(shape[1], 5, replace=False)] *= 1e5
        elif kind == "items":
            B, H = shape[0], shape[2]
            if B == 1:
                g[:, :, :H // 2] *= 2.0 ** -40
                g[:, :, H // 2:] *= 2.0 ** 20
            else:
                g *= np.array([2.0 ** -40, 2.0 ** 20, 1.0])[(np.arange(B) + 1) % 3][:, None, None, None]
        else:
            assert kind == "train", kind
            g = g * 1e-7
    return torch.from_numpy(_fill_mantissa(g, rng))
