"""The split-operand matrix kernels pinned term by term -- TEST INFRASTRUCTURE ONLY.

The bf16x3 kernels (csrc/bf16x3.h: corr_fwd_mfma_bf16x3, corr_bwd_mfma_bf16x3, pyramid_fwd) form every fp32 product from six
partial products, the f16x2 kernels (csrc/f16x2_split.h: correlation_f16x2*.hip) from three.  Their bounds in
tests/corr_contract_ref.py grow with the number of terms n of an output element, 6 n U23 S and 3 n U23 S; on dense inputs that
growth term is hundreds of times larger than one small partial product, so a kernel that loses one (a dropped or mis-paired
product, a stale l image of one staging slot) stays inside.

A product with a zero factor contributes an exact zero to each of its partial products, and adding an exact zero to an fp32
accumulator is exact.  So every bound holds with n replaced by n_nz, the number of the element's terms whose product is not
zero: the same derivation, no new assumption about the matrix cores.  With sparse operands n_nz is 1 .. 4, the bf16x3 bound falls
to about 2^-20 S, and a lost hl / lh product (about 2^-16 S) or mm product (up to 2^-14 S) is far outside.  Where n_nz = 0 the
output is exactly +0.

This file holds n_nz and the bounds with it, the sparse input builders and the tables of cases that the GPU test
(tests/test_gpu_split_terms.py) runs, and sequential-fp32 models of the two schemes with the mutants that the host test
(tests/test_split_terms_host.py) shows the n_nz bound to reject.
"""
import math

import numpy as np
import torch

import corr_contract_ref as R
import corr_pyramid_ref as RP
import lowp_ref as L

CORR = L.CORR
U23 = L.U23
f32 = np.float32


# ------------------------------------------------------------------ the cases (shapes: the smallest that cross each structure)
def params_md(md):
    return (md, 1, md, 1, 2)


X3_FWD_MD = (20, 12)                                         # as test_gpu_f32_contract.MFMA_CASES
X3_FWD_SHAPES = [(1, 32, 8, 16),                             # one stage
                 (1, 64, 8, 20),                             # two stages, partial width
                 (2, 96, 12, 64)]                            # full x tile, two items
X3_ONE_CHANNEL = (0, 7, 8, 24, 31, 32, 63)
X3_BWD_SHAPES = [(1, 64, 8, 20), (1, 128, 12, 36)]           # radius 10, C % 64 == 0, W % 4 == 0; two 32-column tiles, two channel groups
F16_FWD_NARROW, F16_FWD_WIDE = (1, 320, 6, 56), (1, 320, 2, 136)
F16_BWD_SHAPES = [(1, 64, 2, 8), (9, 192, 6, 56), (1, 64, 6, 72), (22, 64, 48, 8)]   # BWD_NARROW[0], [1], BWD_WIDE[0], the multi-task shape


def channel_density(C):
    """Density of channel_sparse for a sum over C channels: n_nz of an output is Binomial(C, d^2); d^2 C = 2.5 puts four outputs in
    five at 1 <= n_nz <= 4."""
    return min(1.0, math.sqrt(2.5 / C))


def terms_in_image(H, W, md=20):
    """Displacements (of stride 2) of a pixel in the middle of the image whose partner lies inside it."""
    D = 2 * (md // 2) + 1
    return min(D, H // 2) * min(D, W // 2)


def term_density(H, W, md=20):
    """Density of grad_sparse (of gradOutput's entries), and of channel_sparse where the sum runs over the displacements (the
    backward with dense gradOutput): 2.5 non-zero terms among those a middle pixel has inside the image, at most every second
    entry.  About 0.6 % at 48 x 64, where all 441 displacements are inside."""
    return min(0.5, 2.5 / terms_in_image(H, W, md))


# ------------------------------------------------------------------ sparse inputs with full 24-bit mantissas
def _x3_bits(x):
    """Bits 15 and 7 of every non-zero value forced on: after h = the upper 16 bits, m holds bit 15 (|m| >= 2^-9 |x|) and l
    holds bit 7 (|l| >= 2^-17 |x|).  Bit 0 is on already (_fill_mantissa)."""
    bits = x.view(np.uint32) | np.uint32(0x8080)
    return np.where(x != 0, bits.view(f32), x)


def _f16_bits(x):
    """Bit 11 := not bit 12.  An f16 step of a (scaled, f16-normal) value is bit 13 of the fp32 mantissa; the 13 bits below it,
    r, then lie in [2048, 6144): l = r or r - 8192 after the round to nearest, |l| >= a quarter of the step."""
    bits = x.view(np.uint32)
    bits = (bits & ~np.uint32(0x800)) | ((~bits >> np.uint32(1)) & np.uint32(0x800))
    return np.where(x != 0, bits.view(f32), x)


def _values(shape, rng, split):
    """Unit-normal values, random low mantissa bits, then the bits that keep the scheme's small terms large."""
    x = R._fill_mantissa(rng.standard_normal(shape), rng).astype(f32)
    return {"bf16x3": _x3_bits, "f16x2": _f16_bits}[split](x)


def dense_pair(shape, seed, split, shape2=None):
    """in1, in2 (or fmap1, fmap2 of spatial size shape2) with every element non-zero."""
    rng = np.random.default_rng(1000 + seed)
    shape2 = shape if shape2 is None else tuple(shape[:2]) + tuple(shape2)
    return torch.from_numpy(_values(shape, rng, split)), torch.from_numpy(_values(shape2, rng, split))


def channel_sparse(shape, density, seed, split, shape2=None):
    """in1, in2 (fmap1, fmap2): every pixel of either keeps its own random subset of the channels, each with probability `density`."""
    rng = np.random.default_rng(2000 + seed)
    shape2 = shape if shape2 is None else tuple(shape[:2]) + tuple(shape2)
    out = []
    for s in (shape, shape2):
        x = _values(s, rng, split)
        out.append(torch.from_numpy(np.where(rng.random(s) < density, x, f32(0))))
    return tuple(out)


def grad_sparse(shape, density, seed, split):
    """gradOutput (B, D^2, oH, oW) that keeps a random subset of its (plane, pixel) entries; in1 and in2 stay dense (dense_pair)."""
    rng = np.random.default_rng(3000 + seed)
    x = _values(shape, rng, split)
    return torch.from_numpy(np.where(rng.random(shape) < density, x, f32(0)))


def one_channel(shape, c, seed, split, shape2=None):
    """in1, in2 with channel c alone non-zero: n_nz <= 1 everywhere, every sum is one product."""
    a, b = dense_pair(shape, seed, split, shape2)
    for t in (a, b):
        keep = t[:, c].clone()
        t.zero_()
        t[:, c] = keep
    return a, b


def dense_grad(shape, seed, split):
    """gradOutput with every entry non-zero."""
    return torch.from_numpy(_values(shape, np.random.default_rng(4000 + seed), split))


def _gshape(shape, md=20):
    B, C, H, W = shape
    return (B,) + L.out_shape(H, W, *params_md(md))


def x3_fwd_inputs(shape):
    """(name, in1, in2) of a bf16x3 forward case."""
    yield ("channel_sparse",) + channel_sparse(shape, channel_density(shape[1]), sum(shape), "bf16x3")
    for c in X3_ONE_CHANNEL:
        if c < shape[1]:
            yield (f"one_channel {c}",) + one_channel(shape, c, c, "bf16x3")


def x3_bwd_inputs(shape):
    """(name, in1, in2, gradOutput) of a bf16x3 backward case: sparse gradOutput against dense in1 / in2, and dense gradOutput against
    channel_sparse in1 / in2 at the displacements' density (n_nz then counts the terms whose X operand is not zero)."""
    B, C, H, W = shape
    d, seed = term_density(H, W), sum(shape)
    yield ("grad_sparse",) + dense_pair(shape, seed, "bf16x3") + (grad_sparse(_gshape(shape), d, seed, "bf16x3"),)
    yield ("channel_sparse",) + channel_sparse(shape, d, seed, "bf16x3") + (dense_grad(_gshape(shape), seed, "bf16x3"),)


def pyramid_inputs(shape):
    """(name, fmap1, fmap2) of a pyramid case; one_channel also at the last channel (of a ragged last stage: C = 40, C = 8)."""
    B, C, (H, W), hw2, _ = shape
    s = (B, C, H, W)
    yield ("channel_sparse",) + channel_sparse(s, channel_density(C), B + C + H + W, "bf16x3", hw2)
    for c in sorted({c for c in X3_ONE_CHANNEL if c < C} | {C - 1}):
        yield (f"one_channel {c}",) + one_channel(s, c, c, "bf16x3", hw2)


def f16_fwd_inputs(shape):
    return channel_sparse(shape, channel_density(shape[1]), sum(shape), "f16x2")


def f16_bwd_inputs(shape):
    """in1, in2 dense, gradOutput grad_sparse."""
    B, C, H, W = shape
    return dense_pair(shape, sum(shape), "f16x2") + (grad_sparse(_gshape(shape), term_density(H, W), sum(shape), "f16x2"),)


# ------------------------------------------------------------------ n_nz per output element
def _ind(x):
    return (x != 0).double()


def nnz_fwd(a, b, params):
    """Terms (channels) of every output of the Correlation forward whose product is not zero, float64 integers."""
    return torch.round(a.shape[1] * L.corr_fwd64(_ind(a), _ind(b), *params))


def nnz_bwd(a, b, go, params):
    """(grad_in1, grad_in2): terms (displacements) whose product gradOutput x in2 / gradOutput x in1 is not zero."""
    C = a.shape[1]
    n1, n2 = L.corr_bwd64(_ind(a), _ind(b), _ind(go), *params)
    return torch.round(C * n1), torch.round(C * n2)


def nnz_pyramid(f1, f2):
    """Level 0 of the pyramid, (B H W) x H2 x W2."""
    B, C, H, W = f1.shape
    n = torch.einsum("bcp,bcq->bpq", _ind(f1).reshape(B, C, -1), _ind(f2).reshape(B, C, -1))
    return torch.round(n).reshape(B * H * W, *f2.shape[2:])


def sole_terms_fwd(a, b, params):
    """The channels that are the only non-zero term (n_nz = 1) of at least one output: the channel index is carried through the
    same sum (weights c + 1), read where n_nz = 1."""
    C = a.shape[1]
    w = torch.arange(1, C + 1, dtype=torch.float64, device=a.device).view(1, C, 1, 1)
    tag = torch.round(C * L.corr_fwd64(_ind(a) * w, _ind(b), *params))
    return set((tag[nnz_fwd(a, b, params) == 1] - 1).long().unique().tolist())


def sole_terms_bwd(a, b, go, params):
    """(grad_in1, grad_in2): the displacement planes that are the only non-zero term of at least one gradient element."""
    C, D2 = a.shape[1], go.shape[1]
    w = torch.arange(1, D2 + 1, dtype=torch.float64, device=a.device).view(1, D2, 1, 1)
    t1, t2 = L.corr_bwd64(_ind(a), _ind(b), _ind(go) * w, *params)
    n1, n2 = nnz_bwd(a, b, go, params)
    pick = lambda t, n: set((torch.round(C * t)[n == 1] - 1).long().unique().tolist())
    return pick(t1, n1), pick(t2, n2)


def reachable_planes(H, W, md=20):
    """The displacement planes with any term inside an H x W image: |dy| <= H - 2 and |dx| <= W - 2 (the parity is kept).  The
    other planes have no term for any input; on the small shapes of the cases they are most of the 441."""
    dr = md // 2
    D = 2 * dr + 1
    return {tj * D + ti for tj in range(D) for ti in range(D) if 2 * abs(tj - dr) < H and 2 * abs(ti - dr) < W}


def sole_terms_pyramid(f1, f2):
    B, C = f1.shape[:2]
    w = torch.arange(1, C + 1, dtype=torch.float64).view(1, C, 1)
    tag = torch.einsum("bcp,bcq->bpq", _ind(f1).reshape(B, C, -1) * w, _ind(f2).reshape(B, C, -1)).reshape(-1, *f2.shape[2:])
    return set((torch.round(tag)[nnz_pyramid(f1, f2) == 1] - 1).long().unique().tolist())


def small_count_fraction(n, any_term):
    """Of the elements with any term inside the image, the fraction at 1 <= n_nz <= 4."""
    return float(((n >= 1) & (n <= 4)).sum()) / max(1, int(any_term.sum()))


# ------------------------------------------------------------------ the bounds with n = n_nz
def delta_x3(ref, absr, n, C):
    """corr_contract_ref.delta_bf16x3 with the count as a tensor; C stays the channel count (the 1/C step, the subnormal floor)."""
    return R.delta_bf16x3(ref, absr, n, C=C)


def delta_f16x2_fwd(ref, absr, s_mb_a, s_ma_b, s_mm, C, n):
    """corr_contract_ref.delta_f16x2_fwd with the count n in the `sums` factor alone (that function takes C for both the count
    and the 1/C step): its three lines restated; test_split_terms_host checks that n = C gives the same numbers.  The split part
    is sparse-aware through its sums."""
    pow2 = (C & (C - 1)) == 0
    split = R.C_REL * absr + R.C_FLOOR * (s_mb_a + s_ma_b) + R.C_MM * s_mm
    sums = 3 * n * U23 * ((1 + 2.0 ** -9) * absr + R.C_FLOOR * (s_mb_a + s_ma_b))
    epi = (0.0 if pow2 else U23) * ref.abs() + (1 if pow2 else 2) * R.F32_SUB
    return split + sums + epi


def fwd_f16x2(a, b, wide, n=None):
    """(ref, delta, n_nz) of the f16x2 forward: the magnitudes and sums of corr_contract_ref.fwd_sums on the same tensors (the
    kernel's sample sees the zeros), the count n_nz (or `n` for all terms)."""
    ref, absr, s1, s2, s3 = R.fwd_sums(a, b, CORR, wide=wide)
    nz = nnz_fwd(a, b, CORR)
    return ref, delta_f16x2_fwd(ref, absr, s1, s2, s3, a.shape[1], nz if n is None else n), nz


def bwd_f16x2(a, b, go, n=None):
    """((r1, d1, n1), (r2, d2, n2)) of the f16x2 backward: corr_contract_ref.bwd_deltas with the count replaced by n_nz (`n`:
    all terms instead).  No operand here is at or above 65520 (asserted): no element is recomputed."""
    params = CORR
    t1, t2 = R.bwd_touched(a, b, go, params)
    assert not bool(t1.any() | t2.any())
    B, C, H, W = a.shape
    mx1, mx2 = R.m_bwd_x(b), R.m_bwd_x(a)
    r1, r2 = L.corr_bwd64(a, b, go, *params)
    ab1, ab2 = L.corr_bwd64(a.abs(), b.abs(), go.abs(), *params)
    mg = R.m_bwd_g(go, H, W)
    ga = go.double().abs()
    ones_x, ones_g = torch.ones_like(a, dtype=torch.float64), torch.ones_like(ga)
    sg1, sg2 = L.corr_bwd64(ones_x, ones_x, ga, *params)
    sb1, _ = L.corr_bwd64(ones_x, b.double().abs(), ones_g, *params)
    _, sa2 = L.corr_bwd64(a.double().abs(), ones_x, ones_g, *params)
    cnt1, cnt2 = L.corr_bwd64(ones_x, ones_x, ones_g, *params)
    n1, n2 = nnz_bwd(a, b, go, params)
    c1, c2 = (n1, n2) if n is None else (n, n)
    d1 = R.delta_f16x2_bwd(r1, ab1, mx1 * sg1, mg * sb1, mx1 * mg * cnt1, c1)
    d2 = R.delta_f16x2_bwd(r2, ab2, mx2 * sg2, mg * sa2, mx2 * mg * cnt2, c2)
    return (r1, d1, n1), (r2, d2, n2)


def pyramid_bounds(levels, S0, C, n):
    """corr_pyramid_ref.bounds with the per-element count n for delta_0 (its two lines restated); the pooled levels follow by
    pool_exact as there."""
    m = RP.header_macros()
    d, S = R.delta_bf16x3(levels[0], S0, n, C=C), S0
    out = [d]
    for l in range(1, len(levels)):
        d, S = RP.pool_exact(d), RP.pool_exact(S)
        out.append(d + l * m["FN2Y_BOUND_PER_POOL"] * S)
    return out


def pooled_counts(n, levels):
    """n_nz summed over the cells of each level's elements: 0 there means that the element is exactly +0."""
    out = [n]
    for _ in range(1, levels):
        out.append(RP.pool_exact(out[-1], weight=1.0))
    return out


def inside(got, ref, delta):
    """(every element of `got` in the fp32 bracket of ref +- delta, worst |got - ref| / delta)."""
    lo, hi = L.bracket(ref, delta, torch.float32)
    ratio = float(((got.double() - ref).abs() / delta.clamp(min=1e-300)).max())
    return not bool(L.outside(got, lo, hi).any()), ratio


def plus_zero_where(got, n):
    """Every element with no non-zero term is +0, bit for bit."""
    return bool((got.contiguous().view(torch.int32)[n.reshape(got.shape) == 0] == 0).all())


# ------------------------------------------------------------------ sequential-fp32 models of the two schemes
ORDER_CORR = ("hh", "hm", "mh", "mm", "hl", "lh")            # PA / PB of corr_fwd_mfma_bf16x3, PG / PN of corr_bwd_mfma_bf16x3
ORDER_PYRAMID = ("mm", "hl", "lh", "hm", "mh", "hh")         # pyramid_fwd: the small terms first
ORDER_F16 = ("hh", "hl", "lh")                               # ah bh, ah bl, al bh
X3_MUTANTS = ("drop_mm", "drop_hl", "drop_lh", "lh_as_hl", "stale_l_slot")
X3_BWD_MUTANTS = ("drop_mm", "drop_hl", "drop_lh", "lh_as_hl", "carry_l")


def split3(x):
    """bf16x3.h split3 on a float32 array: h = the upper 16 bits, m = the upper 16 bits of x - h, l = x - h - m, all exact."""
    x = np.ascontiguousarray(x, f32)
    trunc = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)
    h = trunc(x)
    r = x - h
    m = trunc(r)
    return h, m, r - m


def split2(x):
    """The f16 split at scale exponent 0: h = RNE_f16(x), l = RNE_f16(x - h), as float32 arrays."""
    x = np.ascontiguousarray(x, f32)
    h = x.astype(np.float16).astype(f32)
    return h, (x - h).astype(np.float16).astype(f32)


def accumulate(pair, n_terms, shape, order, kstep, letters="hml", mutant=None):
    """One fp32 accumulator per output element, the terms in steps of `kstep` as one matrix instruction takes them: per step the
    partial products in `order` ("hl": the first operand's h times the second's l), inside a product the step's terms one
    after the other, every add rounded to fp32 (the partial products are exact in fp32).  pair(t) gives the two operands of
    term t as tuples of term arrays in the order of `letters`, broadcastable to `shape`.  The matrix core's own order inside an
    instruction is not known; no bound depends on it.
    mutant: drop_<p> -- product p never issued; lh_as_hl -- hl issued twice in place of lh; stale_l_slot -- the first operand's l
    zero for the terms t with (t % 32) // 8 == 3, the fourth 16-byte staging slot of a 32-channel stage."""
    at = {c: i for i, c in enumerate(letters)}
    acc = np.zeros(shape, f32)
    for t0 in range(0, n_terms, kstep):
        ops = []
        for t in range(t0, min(t0 + kstep, n_terms)):
            a, b = pair(t)
            if not (a[0].any() and b[0].any()):      # an operand that is zero everywhere (h = 0 iff x = 0): only exact zeros to add
                continue
            if mutant == "stale_l_slot" and (t % 32) // 8 == 3:
                a = a[:2] + (np.zeros_like(a[2]),)
            ops.append((a, b))
        for p in order:
            if mutant == "drop_" + p:
                continue
            if mutant == "lh_as_hl" and p == "lh":
                p = "hl"
            i, j = at[p[0]], at[p[1]]
            for a, b in ops:
                acc = acc + a[i] * b[j]
    return acc


def _over_c(acc, C):
    """The 1/C step in fp32: an exact multiply for a power of two, else a division."""
    return acc * f32(1.0 / C) if (C & (C - 1)) == 0 else acc / f32(C)


def model_x3_fwd(a, b, params, mutant=None, order=ORDER_CORR):
    """Correlation forward (k = 1, stride1 = 1, pad = md) by the bf16x3 scheme, numpy float32 (B, D^2, H, W): steps of 32 channels."""
    pad, k, md, s1, s2 = params
    assert k == 1 and s1 == 1 and pad == md
    a, b = a.numpy(), b.numpy()
    B, C, H, W = a.shape
    dr = md // s2
    D = 2 * dr + 1
    at = tuple(t[:, :, None] for t in split3(a))                                     # (B, C, 1, H, W)
    bp = tuple(np.pad(t, ((0, 0), (0, 0), (md, md), (md, md))) for t in split3(b))
    cols = np.arange(W)[None, :] + s2 * np.arange(D)[:, None]                          # (ti, x) -> padded column
    out = np.empty((B, D * D, H, W), f32)
    for tj in range(D):
        bt = tuple(np.ascontiguousarray(t[:, :, s2 * tj:s2 * tj + H][:, :, :, cols].transpose(0, 1, 3, 2, 4)) for t in bp)   # (B, C, ti, H, W)
        pair = lambda c: (tuple(t[:, c] for t in at), tuple(t[:, c] for t in bt))
        out[:, tj * D:(tj + 1) * D] = _over_c(accumulate(pair, C, (B, D, H, W), order, 32, mutant=mutant), C)
    return torch.from_numpy(out)


def _shifted(t, dy, dx, E, H, W):
    return t[..., E + dy:E + dy + H, E + dx:E + dx + W]


def _carry_l(l):
    """carry_l: the l image of every second block of 4 lattice columns (8 pixels of both parities) is the one two blocks
    (16 pixels) to its left -- corr_bwd_mfma_bf16x3 keeps block 2 sl + 2 of a slot as block 0 of the next (hb[T][0] = hb[T][2]);
    zeros where there is none."""
    x = np.arange(l.shape[-1])
    src = np.pad(l, [(0, 0)] * (l.ndim - 1) + [(16, 0)])[..., :l.shape[-1]]
    return np.where((x >> 3) & 1, src, l)


def model_bwd(a, b, go, params, scheme="bf16x3", mutant=None):
    """Both input gradients, numpy float32, by the bf16x3 scheme (six products, ORDER_CORR) or the f16 split at scale exponent 0
    (three: gh xh, gh xl, gl xh; unit-scale data): the D^2 displacement terms of an element in their natural order, in steps
    of 32 (bf16x3: one instruction takes 4 rows x 8 displacement columns, another order of the same terms).  The first
    operand is gradOutput, the second X (in2 for grad_in1, in1 for grad_in2).  Mutants of `accumulate`, carry_l (bf16x3; on X's
    l image) and drop_glxh (f16x2: gl xh never issued)."""
    pad, k, md, s1, s2 = params
    assert k == 1 and s1 == 1 and pad == md
    sp, order, letters = (split3, ORDER_CORR, "hml") if scheme == "bf16x3" else (split2, ORDER_F16, "hl")
    if mutant == "drop_glxh":
        mutant = "drop_lh"
    a, b, go = a.numpy(), b.numpy(), go.numpy()
    B, C, H, W = a.shape
    dr = md // s2
    D = 2 * dr + 1
    E = md
    disp = [(s2 * (tj - dr), s2 * (ti - dr)) for tj in range(D) for ti in range(D)]
    padded = lambda ts: tuple(np.pad(t, ((0, 0), (0, 0), (E, E), (E, E))) for t in ts)

    def x_terms(x):
        ts = sp(x)
        if mutant == "carry_l":
            ts = ts[:2] + (_carry_l(ts[2]),)
        return padded(ts)

    acc_mut = None if mutant == "carry_l" else mutant
    gt, gp = sp(go), padded(sp(go))
    bx, ax = x_terms(b), x_terms(a)
    p1 = lambda d: (tuple(t[:, d, None] for t in gt), tuple(_shifted(t, *disp[d], E, H, W) for t in bx))
    p2 = lambda d: (tuple(_shifted(t[:, d, None], -disp[d][0], -disp[d][1], E, H, W) for t in gp),
                    tuple(_shifted(t, -disp[d][0], -disp[d][1], E, H, W) for t in ax))
    g1 = _over_c(accumulate(p1, D * D, a.shape, order, 32, letters, acc_mut), C)
    g2 = _over_c(accumulate(p2, D * D, a.shape, order, 32, letters, acc_mut), C)
    return torch.from_numpy(g1), torch.from_numpy(g2)


def model_pyramid(f1, f2, levels, mutant=None, order=ORDER_PYRAMID):
    """The levels (B H W) x h x w, float32: level 0 by the bf16x3 scheme in steps of 16 channels (v_mfma_f32_32x32x16_bf16), times
    fl32(1 / sqrt(C)); the pooled levels by corr_pyramid_ref.pool32."""
    B, C, H, W = f1.shape
    H2, W2 = f2.shape[2:]
    at = tuple(t.reshape(B, C, H * W, 1) for t in split3(f1.numpy()))
    bt = tuple(t.reshape(B, C, 1, H2 * W2) for t in split3(f2.numpy()))
    pair = lambda c: (tuple(t[:, c] for t in at), tuple(t[:, c] for t in bt))
    acc = accumulate(pair, C, (B, H * W, H2 * W2), order, 16, mutant=mutant)
    out = [torch.from_numpy(acc * f32(1.0 / math.sqrt(C))).reshape(B * H * W, H2, W2)]
    for _ in range(1, levels):
        out.append(RP.pool32(out[-1]))
    return out
