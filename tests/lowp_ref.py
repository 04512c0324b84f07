"""float64 references and rounding brackets for the half and bfloat16 kernels -- TEST INFRASTRUCTURE ONLY.

The 16-bit correlation and ChannelNorm kernels promise an exact rounding sequence (include/flownet2_hip.h at FN2_BF16 and
FN2_CORR_MFMA_F16X2): products of two 16-bit values are exact in fp32, sums are fp32, every result is rounded to the tensor's
type once.  A kernel that keeps that promise forms an fp32 value within `delta` of the exact result (delta: the fp32 summation
error bound of the operation, per element) and rounds it once; since rounding is monotone its output lies in

    bracket(ref64, delta, dtype) = [RNE_T(RD_f32(ref64 - delta)), RNE_T(RU_f32(ref64 + delta))].

Here ref64 is the operation in float64 (torch ops on whatever device the tensors are on; not the HIP kernels, not the oracle).
The error bounds scale with abs_ref, the same operation on |operands| (sum of |terms| / nelems for each output element), not with
the largest output: a one-ulp-class mistake (a product or partial sum rounded to 16 bits, a 1/C rounded to bf16) leaves the
bracket.  tests/test_lowp_ref_host.py checks the references against the oracle and the bracket on hand-made cases."""
import numpy as np
import torch
import torch.nn.functional as F

U23 = 2.0 ** -23   # fp32 rounding unit, doubled: the bounds hold if the matrix cores' internal sums truncate
CORR = (20, 1, 20, 1, 2)   # FlowNetC's cost volume (FlowNetC.py:28): pad, kernel_size, max_displacement, stride1, stride2


def out_shape(H, W, pad, k, md, s1, s2):
    """nOut, oH, oW of the header's shape math (fn2_correlation_output_shape)."""
    kr = (k - 1) // 2
    D = 2 * (md // s2) + 1
    oH = -(-(H + 2 * pad - 2 * (kr + md)) // s1)
    oW = -(-(W + 2 * pad - 2 * (kr + md)) // s1)
    return D * D, oH, oW


def _displacements(md, s2):
    dr = md // s2
    return [(tj * s2, ti * s2) for tj in range(-dr, dr + 1) for ti in range(-dr, dr + 1)]


def _box(x, kr):
    """Sum over the (2 kr + 1)^2 window centred on each element of (B, h, w), zeros outside."""
    if kr == 0:
        return x
    kw = 2 * kr + 1
    return F.conv2d(x[:, None], torch.ones(1, 1, kw, kw, dtype=x.dtype, device=x.device), padding=kr)[:, 0]


def corr_fwd64(a, b, pad, k, md, s1, s2, prod=None):
    """Correlation forward in float64: out[n, (tj, ti), oy, ox] = sum_{j, i, c} a[c, y + j, x + i] * b[c, y + j + tj*s2, x + i +
    ti*s2] / (k*k*C) with (y, x) = (oy*s1 + md - pad, ox*s1 + md - pad) in image coordinates; every read outside the image is zero
    (the zero padding, and beyond it the header's definition of the reference's out-of-buffer reads).  `prod(a, b)`: an optional
    replacement of the product (the host tests simulate wrong kernels with it)."""
    B, C, H, W = a.shape
    nOut, oH, oW = out_shape(H, W, pad, k, md, s1, s2)
    kr = (k - 1) // 2                                  # window radius (an even k sums one (2 kr + 1)^2 window, as the reference)
    E = pad + md + k                                   # canvas margin around the image
    a64 = F.pad(a.double(), (E, E, E, E))
    b64 = F.pad(b.double(), (E, E, E, E))
    Lh, Lw = (oH - 1) * s1 + 2 * kr + 1, (oW - 1) * s1 + 2 * kr + 1   # rows / columns the windows of all outputs cover
    y0, x0 = E + md - pad - kr, E + md - pad - kr      # canvas position of the first window's corner
    out = torch.empty(B, nOut, oH, oW, dtype=torch.float64, device=a.device)
    pa = a64[:, :, y0:y0 + Lh, x0:x0 + Lw]
    for d, (j2, i2) in enumerate(_displacements(md, s2)):
        pb = b64[:, :, y0 + j2:y0 + j2 + Lh, x0 + i2:x0 + i2 + Lw]
        p = (pa * pb if prod is None else prod(pa, pb)).sum(1)
        out[:, d] = _box(p, kr)[:, kr::s1, kr::s1][:, :oH, :oW]
    return out / (k * k * C)


def corr_bwd64(a, b, go, pad, k, md, s1, s2):
    """Both input gradients of corr_fwd64 in float64 (stride1 = 1, the only stride the backward defines): for every displacement,
    the k x k window sums of gradOutput times the displaced other input, / (k*k*C)."""
    assert s1 == 1, "the backward is defined for stride1 = 1 only"
    B, C, H, W = a.shape
    nOut, oH, oW = out_shape(H, W, pad, k, md, s1, s2)
    kr = (k - 1) // 2
    E = pad + md + k
    a64 = F.pad(a.double(), (E, E, E, E))
    b64 = F.pad(b.double(), (E, E, E, E))
    # S[y, x]: sum of gradOutput over the outputs whose window covers image position (y, x), for each displacement; output (oy,
    # ox) is centred at image (oy + md - pad, ox + md - pad).  Canvas in image coordinates with margin E on every side.
    g1 = torch.zeros(B, C, H, W, dtype=torch.float64, device=a.device)
    g2 = torch.zeros_like(g1)
    go64 = go.double()
    cy, cx = E + md - pad, E + md - pad
    for d, (j2, i2) in enumerate(_displacements(md, s2)):
        canvas = torch.zeros(B, H + 2 * E, W + 2 * E, dtype=torch.float64, device=a.device)
        canvas[:, cy:cy + oH, cx:cx + oW] = go64[:, d]
        S = _box(canvas, kr)                                           # image (y, x) at canvas (E + y, E + x)
        s1v = S[:, None, E:E + H, E:E + W]
        g1 += s1v * b64[:, :, E + j2:E + j2 + H, E + i2:E + i2 + W]
        s2v = S[:, None, E - j2:E - j2 + H, E - i2:E - i2 + W]          # windows of the outputs that read in2 at (y, x)
        g2 += s2v * a64[:, :, E - j2:E - j2 + H, E - i2:E - i2 + W]
    return g1 / (k * k * C), g2 / (k * k * C)


# ------------------------------------------------------------------ error bounds (one per documented contract)
def delta_fwd(ref, abs_ref, C, k=1):
    """Matrix kernels and the bf16 general kernel: exact products, fp32 sum of n = C*k*k terms, the 1/C step."""
    return (C * k * k) * U23 * abs_ref + U23 * ref.abs()


def delta_fwd_direct_half(ref, abs_ref, C, k=1):
    """The half general kernel rounds every product to half (fwd_prod in correlation_direct.hip, as the reference does): 2^-11
    relative per product, and at most half of the smallest subnormal step (2^-25) absolute where a product is below 2^-14."""
    return delta_fwd(ref, abs_ref, C, k) + 2.0 ** -11 * abs_ref + 2.0 ** -25


def n_bwd(md, s2, k):
    """Terms of one input-gradient element: (displacement, window pixel) pairs."""
    D = 2 * (md // s2) + 1
    return D * D * k * k


def delta_bwd(ref, abs_ref, md=20, s2=2, k=1):
    """16-bit backward kernels (matrix and general): exact products, fp32 sums, the 1/C step."""
    return n_bwd(md, s2, k) * U23 * abs_ref + U23 * ref.abs()


def _f16x2_magnitudes(x, block=8):
    """Upper bound of the f16x2 backward's per-channel typical magnitude m for every element: the scale comes from a sample of the
    channel taken inside the task's centre rows (an aligned block of 8 rows), so m <= the largest |value| of the channel in that
    block; a sample without non-zero values leaves the operand unscaled (m = 2^-1)."""
    ax = x.double().abs()
    m = torch.empty_like(ax)
    for y0 in range(0, x.shape[2], block):
        blk = ax[:, :, y0:y0 + block]
        bm = blk.amax(dim=(2, 3), keepdim=True)
        bm = torch.where((blk == 0).flatten(2).any(2)[..., None, None], bm.clamp(min=0.5), bm)
        m[:, :, y0:y0 + block] = bm
    return m


def delta_bwd_widened(a, b, go, r1, r2, ab1, ab2, md=20, s2=2):
    """Wide (W > 64) half / bf16 backward: the binding widens to fp32, runs the fp32 f16x2 kernel and rounds once.  The header's
    per-operand bound of that kernel is max(2^-22 |x| / m, 2^-24) relative to m, m the operand's typical magnitude (per channel
    for in1 / in2, per task for gradOutput).  Per gradient element that is a relative term 2^-21 abs_ref (two operands) plus the
    floor 2^-24 m times the sum of the other operand's magnitudes over the element's terms; the fp32 sums add 3n terms (three
    partial products each)."""
    pad, k, s1 = md, 1, 1
    ga = go.double().abs()
    mg = torch.clamp(ga.flatten(1).amax(1), min=0.0)
    mg = torch.where((ga.flatten(1) == 0).any(1), mg.clamp(min=0.5), mg).view(-1, 1, 1, 1)
    ones_x = torch.ones_like(a, dtype=torch.float64)
    ones_g = torch.ones_like(go, dtype=torch.float64)
    sg1, sg2 = corr_bwd64(ones_x, ones_x, ga, pad, k, md, s1, s2)            # sum |go| over each element's terms (/ nelems)
    sb1, _ = corr_bwd64(ones_x, b.double().abs(), ones_g, pad, k, md, s1, s2)  # sum |in2| over the terms of g1
    _, sa2 = corr_bwd64(a.double().abs(), ones_x, ones_g, pad, k, md, s1, s2)  # sum |in1| over the terms of g2
    n3 = 3 * n_bwd(md, s2, k)
    d1 = 2.0 ** -21 * ab1 + 2.0 ** -24 * (_f16x2_magnitudes(b) * sg1 + mg * sb1) + n3 * U23 * ab1 + U23 * r1.abs()
    d2 = 2.0 ** -21 * ab2 + 2.0 ** -24 * (_f16x2_magnitudes(a) * sg2 + mg * sa2) + n3 * U23 * ab2 + U23 * r2.abs()
    return d1, d2


# ------------------------------------------------------------------ the bracket
def _f32_down(x64):
    x = x64.float()
    return torch.where(x.double() > x64, torch.nextafter(x, torch.full_like(x, -float("inf"))), x)


def _f32_up(x64):
    x = x64.float()
    return torch.where(x.double() < x64, torch.nextafter(x, torch.full_like(x, float("inf"))), x)


def bracket(ref64, delta, dtype, post=None):
    """(lo, hi) in `dtype` (torch.float16 / torch.bfloat16): every fp32 value within delta of ref64, rounded once to dtype.
    1. ref64 - delta rounded down, ref64 + delta rounded up to float32 (cast, then nextafter outward where the cast went inward);
    2. `post`, if given: the kernel's monotone fp32 epilogue step (the fused LeakyReLU), applied to both ends;
    3. torch's float32 -> 16-bit conversion, one round to nearest even; a bound past the type's overflow threshold (65520 for
       half) becomes +-inf there.
    Never float64 -> 16 bits directly: torch goes through float32 and would round twice."""
    ref64 = ref64.double()
    delta = torch.as_tensor(delta, dtype=torch.float64, device=ref64.device)
    lo32, hi32 = _f32_down(ref64 - delta), _f32_up(ref64 + delta)
    if post is not None:
        lo32, hi32 = post(lo32), post(hi32)
    return lo32.to(dtype), hi32.to(dtype)


def leaky_matrix(slope, dtype):
    """Fused LeakyReLU of the matrix kernels (correlation_f16_fwd.hip): the slope applied in fp32 to acc / C, then one rounding."""
    def post(x):
        s = torch.tensor(slope, dtype=torch.float32, device=x.device)
        return torch.where(x > 0, x, x * s)
    return post


def leaky_general(slope, dtype):
    """Fused LeakyReLU of the general kernel (corr_fwd_direct): acc / nelems rounded to T, times the slope in fp32, rounded again."""
    def post(x):
        s = torch.tensor(slope, dtype=torch.float32, device=x.device)
        return torch.where(x > 0, x, x.to(dtype).float() * s)
    return post


def outside(got, lo, hi):
    """Mask of elements outside [lo, hi] (NaN is outside)."""
    g = got.float()
    return ~((g >= lo.float()) & (g <= hi.float()))


def check_bracket(got, lo, hi, what=""):
    bad = outside(got, lo, hi)
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements outside the bracket; first at flat index {i}: "
                             f"got {float(got.flatten()[i])!r}, bracket [{float(lo.flatten()[i])!r}, {float(hi.flatten()[i])!r}]")


# ------------------------------------------------------------------ ChannelNorm
def chnorm_fwd_bracket(x, dtype):
    """fn2_channelnorm_forward on 16-bit x: sqrt of an fp32 sum of squares, rounded once.  Half squares are rounded to half first
    (chnorm_sq, as the reference :56; the fp32 product of two halves is exact, so rounding it to half is that one rounding); bf16
    squares are exact.  Bound: C*2^-24 relative on the sum (non-negative terms) is half of that on the sqrt, plus the sqrt's own
    rounding; doubled as everywhere here."""
    xf = x.float()
    sq = xf * xf
    if dtype == torch.float16:
        sq = sq.half().float()
    s = sq.double().sum(1, keepdim=True)
    ref = s.sqrt()
    C = x.shape[1]
    return bracket(ref, (C * 2.0 ** -24 + U23) * ref, dtype)


def chnorm_bwd_bracket(x, out, go):
    """fn2_channelnorm_backward (chnorm_grad, fn2_common.h): float(go) * float(x) in fp32, divided in double by double(out) + 1e-9,
    rounded to float, then to T: two fp32-class roundings (2^-23 relative, plus the double steps and an fp32 underflow floor)."""
    ref = go.double() * x.double() / (out.double() + 1e-9)
    return bracket(ref, (U23 + 2.0 ** -40) * ref.abs() + 2.0 ** -149 / (out.double() + 1e-9), x.dtype)


# ------------------------------------------------------------------ input families
def family_inputs(family, shape, dtype, seed):
    """in1, in2 (CPU, dtype) of input family 1..5:
      1 unit normal;
      2 per-channel scales log-uniform over 2^+-20 (bf16) / 2^+-4 (half), independently for each input;
      3 LeakyReLU(0.1) of a normal: mostly positive, heavy negative tail scaled down;
      4 cancellation: in2 is in1 with the sign flipped on half the channels;
      5 magnitude ramp along the rows over 2^+-12 (bf16) / 2^+-3 (half).
    Half magnitudes keep every product a general kernel rounds to half inside half's range."""
    B, C, H, W = shape
    bf = dtype == torch.bfloat16
    rng = np.random.default_rng(seed * 10 + family)
    a = rng.standard_normal(shape)
    b = rng.standard_normal(shape)
    if family == 2:
        e = 20.0 if bf else 4.0
        a = a * 2.0 ** rng.uniform(-e, e, (1, C, 1, 1))
        b = b * 2.0 ** rng.uniform(-e, e, (1, C, 1, 1))
    elif family == 3:
        a = np.where(a > 0, a, 0.1 * a)
        b = np.where(b > 0, b, 0.1 * b)
    elif family == 4:
        s = np.ones(C)
        s[rng.permutation(C)[:C // 2]] = -1.0
        b = a * s[None, :, None, None]
    elif family == 5:
        e = 12.0 if bf else 3.0
        r = 2.0 ** (e * (2.0 * np.arange(H) / max(H - 1, 1) - 1.0))
        a = a * r[None, None, :, None]
        b = b * r[None, None, :, None]
    else:
        assert family == 1, family
    return (torch.from_numpy(a.astype(np.float32)).to(dtype), torch.from_numpy(b.astype(np.float32)).to(dtype))


def grad_output(kind, shape, dtype, seed):
    """gradOutput (CPU, dtype): 'normal'; 'leaky' -- times a LeakyReLU(0.1) mask (x0.1 on about half the elements); 'window' --
    zero outside a window of displacements and pixels."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(shape)
    if kind == "leaky":
        g = g * np.where(rng.random(shape) < 0.5, 0.1, 1.0)
    elif kind == "window":
        B, N, H, W = shape
        m = np.zeros(shape)
        m[:, N // 4:3 * N // 4, H // 4:H // 4 + max(1, H // 2), W // 4:W // 4 + max(1, W // 2)] = 1.0
        g = g * m
    else:
        assert kind == "normal", kind
    return torch.from_numpy(g.astype(np.float32)).to(dtype)
