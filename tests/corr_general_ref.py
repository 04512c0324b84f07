"""The parameter-general correlation kernels off FlowNetC's configuration -- TEST INFRASTRUCTURE ONLY.

1. GRID: the parameter sets and shapes on which tests/test_corr_general_host.py (CPU) and tests/test_gpu_corr_general.py (GPU) pin
   corr_fwd_direct / corr_bwd_direct (csrc/correlation_direct.hip) per element.
2. model_fwd / model_bwd: those two kernels restated in numpy, operation by operation in the kernel's own types and order, with
   plausible indexing mistakes selectable by `mutation=` (MUTATIONS): the host test shows that the correct model meets the bounds
   of tests/corr_contract_ref.py on the whole grid and that every mutation leaves them on some grid case.
3. The launch predicates of the fp32 matrix kernels (csrc/correlation_mfma.hip corr_forward_mfma_f32, csrc/correlation_mfma_bwd.hip
   corr_backward_mfma_f32) restated, so that a test can say which kernel a call reached.
"""
import numpy as np
import torch

import lowp_ref as L

# ((pad, kernel_size, max_displacement, stride1, stride2), (B, C, H, W)) and what the case is there for
GRID = [
    ((0, 1, 0, 1, 1), (2, 5, 3, 7)),       # md 0: one displacement, no padding, C % 4 == 1
    ((0, 3, 0, 1, 1), (1, 6, 5, 9)),       # md 0 with a 3 x 3 window and no padding: the output is smaller than the map
    ((2, 1, 4, 1, 1), (2, 7, 11, 13)),     # pad < md, dense displacements, C % 4 == 3
    ((6, 1, 4, 1, 2), (1, 3, 5, 6)),       # pad > md: the output is larger than the map
    ((3, 5, 3, 1, 3), (2, 9, 9, 12)),      # k 5, stride2 3 == md
    ((4, 3, 5, 1, 2), (1, 33, 7, 10)),     # md % s2 != 0 with k 3, C = 4 * 8 + 1
    ((4, 2, 4, 1, 3), (2, 4, 6, 8)),       # even k (window radius (k - 1) / 2 = 0, nelems 4 C), md % s2 != 0
    ((7, 3, 7, 1, 3), (1, 70, 4, 5)),      # C = 4 * 17 + 2 next to k 3, md % s2 != 0
    ((3, 3, 4, 2, 2), (2, 5, 13, 17)),     # stride1 2 (forward only), pad < md
    ((5, 1, 5, 3, 2), (1, 6, 10, 14)),     # stride1 3 (forward only), md % s2 != 0 with k 1
    ((1, 3, 2, 3, 1), (2, 2, 9, 16)),      # stride1 3 with k 3 and dense displacements
    ((20, 1, 20, 1, 2), (1, 5, 1, 1)),     # FlowNetC's parameters on a single pixel: one in-image term out of 441
    ((4, 1, 4, 1, 1), (1, 2, 1, 70)),      # a single row, wider than one wave
    ((0, 1, 2, 1, 2), (1, 4, 5, 5)),       # no padding at all: a 1 x 1 output
    ((4, 3, 4, 1, 2), (2, 5, 6, 9)),       # md - (md / s2) s2 < kr: the reference reads outside its padded buffer (defined as 0)
    ((6, 5, 6, 1, 3), (1, 3, 6, 8)),       # the same regime with k 5
    ((9, 1, 3, 1, 2), (1, 2, 2, 3)),       # pad three times md on a 2 x 3 map: most outputs see only padding
    ((0, 1, 1, 1, 1), (1, 1, 3, 3)),       # one channel, a 1 x 1 output
    ((2, 3, 2, 2, 2), (1, 2, 4, 4)),       # stride1 2 with k 3 on a 4 x 4 map
]
EMPTY = ((6, 5, 6, 1, 3), (1, 3, 4, 7))   # H + 2 pad - 2 (kr + md) == 0: fn2_correlation_output_shape returns FN2_EINVAL

# the kernel's launch constants (csrc/correlation_direct.hip fwd_direct_launch / bwd_direct_launch: stream_grid(total, 256L * 64))
GRID_CAP_BLOCKS, BLOCK = 256 * 64, 256

# mutation -> what a kernel with that mistake would do
MUTATIONS = {
    "off_sign": "forward: y1 = by s1 + pad - md (the sign of md - pad)",
    "pad_is_md": "forward: y1 = by s1 (pad == md assumed)",
    "tj_ti": "forward: tj = tc % D - dr, ti = tc / D - dr (swapped)",
    "nelems": "forward and backward: nelems = k C",
    "g2_window": "backward: grad_input2's window displaced by +i2 / +j2 instead of -i2 / -j2",
    "kr": "forward and backward: kr = k / 2 (wrong for an even k)",
    # further mistakes the kernel's text invites
    "s1_ignored": "forward: y1 = by + md - pad (stride1 dropped)",
    "leftover": "forward: the C % 4 leftover channels dropped",
    "bwd_tj_ti": "backward: i2 / j2 swapped",
    "bwd_pad_is_md": "backward: the other input read at y + j2 - md (pad == md assumed)",
    "bwd_s2_ignored": "backward: i2 = tc % D - dr (stride2 dropped)",
}
FWD_MUTATIONS = ("off_sign", "pad_is_md", "tj_ti", "nelems", "kr", "s1_ignored", "leftover")
BWD_MUTATIONS = ("nelems", "g2_window", "kr", "bwd_tj_ti", "bwd_pad_is_md", "bwd_s2_ignored")


def case_id(case):
    (pad, k, md, s1, s2), shape = case
    return f"p{pad}k{k}md{md}s{s1}{s2}-" + "x".join(map(str, shape))


def _gather(x, c, ys, xs, H, W):
    """x[:, c, ys, xs] with the indices clipped into the image (the caller masks what lay outside): (B,) + ys.shape."""
    return x[:, c][:, np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)]


def model_fwd(a, b, params, mutation=None):
    """corr_fwd_direct<T> for T = float (numpy float32 inputs) or double (float64 inputs): per (window pixel, displacement) pair
    fwd_channel_sum's four fp32 chains over c = 0, 1, 2, 3 (mod 4) with every product formed in T and rounded to float, the
    C % 4 leftover channels on the first chain, (s0 + s1) + (s2 + s3); one fp32 add per window pixel, j outer and i inner, pairs
    with either pixel outside the image skipped; acc / (k k C) in fp32, stored as T."""
    pad, k, md, s1, s2 = params
    B, C, H, W = a.shape
    f = np.float32
    nOut, oH, oW = L.out_shape(H, W, *params)
    kr = k // 2 if mutation == "kr" else (k - 1) // 2
    dr = md // s2
    D = 2 * dr + 1
    tc = np.arange(nOut)
    tj, ti = (tc % D - dr, tc // D - dr) if mutation == "tj_ti" else (tc // D - dr, tc % D - dr)
    off = {"off_sign": pad - md, "pad_is_md": 0}.get(mutation, md - pad)
    st = 1 if mutation == "s1_ignored" else s1
    y1 = (np.arange(oH) * st + off)[None, :, None] + np.zeros((nOut, 1, oW), np.int64)
    x1 = (np.arange(oW) * st + off)[None, None, :] + np.zeros((nOut, oH, 1), np.int64)
    y2, x2 = y1 + tj[:, None, None] * s2, x1 + ti[:, None, None] * s2
    acc = np.zeros((B, nOut, oH, oW), f)
    with np.errstate(all="ignore"):
        for j in range(-kr, kr + 1):
            for i in range(-kr, kr + 1):
                ya, yb, xa, xb = y1 + j, y2 + j, x1 + i, x2 + i
                valid = (ya >= 0) & (ya < H) & (yb >= 0) & (yb < H) & (xa >= 0) & (xa < W) & (xb >= 0) & (xb < W)
                prod = lambda c: (_gather(a, c, ya, xa, H, W) * _gather(b, c, yb, xb, H, W)).astype(f)   # in T, then to float
                s = [np.zeros_like(acc) for _ in range(4)]
                c = 0
                while c + 4 <= C:
                    for q in range(4):
                        s[q] = s[q] + prod(c + q)
                    c += 4
                while c < C and mutation != "leftover":
                    s[0] = s[0] + prod(c)
                    c += 1
                acc = np.where(valid[None], acc + ((s[0] + s[1]) + (s[2] + s[3])), acc)
        nelems = k * C if mutation == "nelems" else k * k * C
        return (acc / f(nelems)).astype(a.dtype)


def _window_sum(g, ymin, xmin, kr, oH, oW, A):
    """sum of g (B, oH, oW) over rows ymin .. ymin + 2 kr and columns xmin .. xmin + 2 kr clamped to the output, j outer and i
    inner, sequentially in A: (B,) + the broadcast shape of ymin and xmin."""
    shape = np.broadcast(ymin, xmin).shape
    w = np.zeros((g.shape[0],) + shape, A)
    for dj in range(2 * kr + 1):
        for di in range(2 * kr + 1):
            j, i = ymin + dj, xmin + di
            valid = (j >= 0) & (j < oH) & (i >= 0) & (i < oW)
            v = g[:, np.clip(j, 0, oH - 1), np.clip(i, 0, oW - 1)]
            w = np.where(np.broadcast_to(valid, shape)[None], w + v.astype(A), w)
    return w


def model_bwd(a, b, go, params, mutation=None):
    """corr_bwd_direct<T>, stride1 = 1, T = float (accumulating in float) or double (Acc<double>: in double): per displacement
    the window's gradOutput summed first (j outer, i inner), one product with the other input's pixel, added to a sequential
    sum over the displacements in ascending tc; terms whose pixel lies outside the image or whose window holds no output are
    skipped; sum / (k k C) stored as T."""
    pad, k, md, s1, s2 = params
    assert s1 == 1
    B, C, H, W = a.shape
    A = np.float64 if a.dtype == np.float64 else np.float32
    nOut, oH, oW = L.out_shape(H, W, *params)
    kr = k // 2 if mutation == "kr" else (k - 1) // 2
    dr = md // s2
    D = 2 * dr + 1
    y, x = (np.arange(H) + pad)[:, None], (np.arange(W) + pad)[None, :]
    opad = md if mutation == "bwd_pad_is_md" else pad
    sum1, sum2 = np.zeros((B, C, H, W), A), np.zeros((B, C, H, W), A)
    with np.errstate(all="ignore"):
        for tc in range(nOut):
            i2, j2 = (tc % D - dr), (tc // D - dr)
            if mutation == "bwd_tj_ti":
                i2, j2 = j2, i2
            if mutation != "bwd_s2_ignored":
                i2, j2 = i2 * s2, j2 * s2
            g = go[:, tc]
            # grad_input1: one window for every tc, in2 displaced by (+j2, +i2)
            ymin, xmin = y - kr - md, x - kr - md
            has = (ymin + 2 * kr >= 0) & (xmin + 2 * kr >= 0) & (ymin < oH) & (xmin < oW)
            yy, xx = y + j2 - opad, x + i2 - opad
            inimg = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            w = _window_sum(g, ymin, xmin, kr, oH, oW, A)
            v2 = b[:, :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(A)
            sum1 = np.where((has & inimg)[None, None], sum1 + w[:, None] * v2, sum1)
            # grad_input2: the window moves against the displacement, in1 displaced by (-j2, -i2)
            sg = -1 if mutation == "g2_window" else 1
            ymin, xmin = y - kr - md - sg * j2, x - kr - md - sg * i2
            has = (ymin + 2 * kr >= 0) & (xmin + 2 * kr >= 0) & (ymin < oH) & (xmin < oW)
            yy, xx = y - j2 - opad, x - i2 - opad
            inimg = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            w = _window_sum(g, ymin, xmin, kr, oH, oW, A)
            v1 = a[:, :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(A)
            sum2 = np.where((has & inimg)[None, None], sum2 + w[:, None] * v1, sum2)
        nelems = A(k * C if mutation == "nelems" else k * k * C)
        return (sum1 / nelems).astype(a.dtype), (sum2 / nelems).astype(a.dtype)


def inside(got, ref, delta, dtype=torch.float32):
    """(every element of the numpy array `got` lies in lowp_ref.bracket(ref, delta), the worst |got - ref| / delta); float64
    `got` (the double backward) is compared in float64 directly, there is nothing to round to."""
    g = torch.from_numpy(np.ascontiguousarray(got))
    if g.dtype == torch.float64 and dtype == torch.float64:
        lo, hi = ref - delta, ref + delta
        ok = bool(((g >= lo) & (g <= hi)).all())
    else:
        lo, hi = L.bracket(ref, delta, dtype)
        ok = not bool(L.outside(g.to(dtype), lo, hi).any())
    ratio = float(((g.double() - ref).abs() / delta.clamp(min=1e-300)).max()) if g.numel() else 0.0
    return ok, ratio


# ------------------------------------------------------------------ which fp32 matrix kernel a call reaches
def mfma_nv(md):
    """B blocks per A block and axis of the fp32 matrix kernels (corr_forward_mfma_f32: NV = 1 + (dr + 1) / 2, dr = md / 2)."""
    return 1 + (md // 2 + 1) // 2


def mfma_x_tiles(W):
    return (W + 63) // 64          # mf::TILE_X = mb::TILE_X = 64


def mfma_fwd_x4(W, md):
    """mf::launch's 16-byte staging branch (x4 = true), for 16-byte aligned inputs: an even radius and W % 4 == 0."""
    return (md // 2) % 2 == 0 and W % 4 == 0


def bf16x3_fwd_accepts(C, W, md):
    """corr_forward_mfma_f32's bf16x3_ok for 16-byte aligned inputs: dma_ok (an even radius, W % 4 == 0), one x tile, C % 32 == 0."""
    return mfma_fwd_x4(W, md) and mfma_x_tiles(W) == 1 and C % 32 == 0


def bwd_groups64(B, C, H, W, tune=6):
    """Whether corr_backward_mfma_f32 runs 64-channel groups (mb::launch_nv<4>) rather than 32-channel groups (launch_nv<2>):
    tune 6 = FN2_CORR_MFMA_F32 (the occupancy test), 1 = force 32 (debug algo 101), 2 = 64 where C % 64 == 0 (debug algo 102).
    The occupancy test: with one workgroup per CU on 256 CUs, keep 64 unless 32-channel groups fill the last round of
    workgroups more than 1.1 times as well."""
    NRG = (H // 2 + 3) // 4
    base = B * 2 * NRG * mfma_x_tiles(W) * 2

    def round_eff(t):
        r = (t + 255) // 256
        return t / (r * 256) if r else 1.0

    g64 = C % 64 == 0 and tune != 1
    if g64 and tune == 6 and round_eff(base * (C // 32)) > 1.1 * round_eff(base * (C // 64)):
        g64 = False
    return g64
