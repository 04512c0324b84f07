"""float64 reference of ConvexUpsample (include/flownet2_hip_upsample.h), written from the header's formulas on the 7-D view
B x 9 x f x f x H x W of the mask -- not from the kernels' tiling; and ``compose``, RAFT's softmax / unfold / sum / permute
composition in torch.  Test infrastructure only.  The fp32 / 16-bit input values are taken as exact.

    p_k  = softmax_k(mask[b, k f^2 + i f + j, y, x]),   a_k = m_k - max_k m_k,   A = sum_k p_k |a_k|
    v_ck = scale * flow[b, c, y + ky - 1, x + kx - 1]   (a tap outside the image is absent)
    out[b, c, f y + i, f x + j] = sum_k p_k v_ck

Per element the functions return the exact value, the sums the header's bounds are made of, and the number of terms.
"""
import os
import re

import numpy as np

U23 = 2.0 ** -23
SUB = 2.0 ** -149

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flownet2_hip_upsample.h")


def header_macros():
    """The integer macros of the header: FN2U_ABI_VERSION, FN2U_MAX_CHANNELS, FN2U_TILE, FN2U_K0_F, FN2U_K0_M, FN2U_K0_G."""
    txt = open(_HDR).read()
    return {k: int(v) for k, v in re.findall(r"^#define (FN2U_[A-Z0-9_]+) (\d+)\s*$", txt, flags=re.M)}


def groups(f):
    """FN2U_GROUPS(f)"""
    return min(f, 4)


def _softmax(mask, f):
    """p, |a|, A of a B x 9 f^2 x H x W mask, each B x 9 x f x f x H x W (A: B x 1 x ...)."""
    m = np.asarray(mask, dtype=np.float64)
    B, _, H, W = m.shape
    m = m.reshape(B, 9, f, f, H, W)
    a = m - m.max(1, keepdims=True)
    e = np.exp(a)
    p = e / e.sum(1, keepdims=True)
    return p, np.abs(a), (p * np.abs(a)).sum(1, keepdims=True)


def _taps(flow, scale):
    """v: B x C x 9 x H x W (0 for an absent tap), present: 9 x H x W."""
    fl = np.asarray(flow, dtype=np.float64)
    B, C, H, W = fl.shape
    pad = np.zeros((B, C, H + 2, W + 2))
    pad[:, :, 1:-1, 1:-1] = scale * fl
    inside = np.zeros((H + 2, W + 2), dtype=bool)
    inside[1:-1, 1:-1] = True
    v = np.stack([pad[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W] for k in range(9)], 2)
    present = np.stack([inside[k // 3:k // 3 + H, k % 3:k % 3 + W] for k in range(9)], 0)
    return v, present


def _fine(t6):
    """B x C x f x f x H x W (sub-row, sub-column, y, x) -> B x C x f H x f W"""
    B, C, f, _, H, W = t6.shape
    return np.ascontiguousarray(t6.transpose(0, 1, 4, 2, 5, 3)).reshape(B, C, f * H, f * W)


def _coarse(t, f):
    """the inverse of _fine"""
    B, C, fH, fW = t.shape
    return t.reshape(B, C, fH // f, f, fW // f, f).transpose(0, 1, 3, 5, 2, 4)


def forward(flow, mask, f, scale):
    """(exact, S, Sa, n): float64 B x C x f H x f W; S = sum_k p_k |v_ck|, Sa = sum_k p_k |v_ck| (|a_k| + A), n = taps present."""
    p, aa, A = _softmax(mask, f)
    v, present = _taps(flow, scale)
    pe, ve = p[:, None], v[:, :, :, None, None]                    # B x 1 x 9 x f x f x H x W, B x C x 9 x 1 x 1 x H x W
    out = (pe * ve).sum(2)
    S = (pe * np.abs(ve)).sum(2)
    Sa = (pe * np.abs(ve) * (aa + A)[:, None]).sum(2)
    n = np.broadcast_to(present.sum(0)[None, None, None, None], out.shape)
    return _fine(out), _fine(S), _fine(Sa), _fine(n)


def delta_forward(S, Sa, scale):
    k0 = header_macros()["FN2U_K0_F"]
    return U23 * (k0 * S + Sa) + k0 * SUB * max(1.0, abs(scale))


def backward(flow, mask, gout, f, scale):
    """((gflow, Sg, Sga, n), (gmask, Bm0, Bm1)), float64.
    grad_flow's bound is 2^-23 (K0_G Sg + Sga) with Sg = |scale| sum p_k |gO|, Sga = |scale| sum p_k |gO| (|a_k| + A) over its
    n terms; grad_mask's is 2^-23 (K0_M Bm0 + Bm1) with Bm0 = p_k (D_k + sum_k' p_k' D_k') and Bm1 the header's logit terms."""
    p, aa, A = _softmax(mask, f)
    v, present = _taps(flow, scale)
    B, C, _, H, W = v.shape
    g6 = _coarse(np.asarray(gout, dtype=np.float64), f)            # B x C x f x f x H x W
    prod = g6[:, :, None] * v[:, :, :, None, None]                 # B x C x 9 x f x f x H x W
    d, D = prod.sum(1), np.abs(prod).sum(1)                        # B x 9 x f x f x H x W
    dbar = (p * d).sum(1, keepdims=True)
    Sg = (p * D).sum(1, keepdims=True)
    Sga = (p * D * aa).sum(1, keepdims=True)
    gm = p * (d - dbar)
    Bm0 = p * (D + Sg)
    Bm1 = p * ((D + Sg) * (aa + A) + A * Sg + Sga)
    shape = (B, 9 * f * f, H, W)
    # T[b, c, k, y, x] and its bound sums, then the gather of the header
    pg = p[:, None] * np.abs(g6[:, :, None])
    T = (p[:, None] * g6[:, :, None]).sum((3, 4))                  # B x C x 9 x H x W
    Ts, Tsa = pg.sum((3, 4)), (pg * (aa + A)[:, None]).sum((3, 4))

    def gather(t):
        tp = np.zeros((B, C, 9, H + 2, W + 2))
        tp[..., 1:-1, 1:-1] = t
        return sum(tp[:, :, k, 2 - k // 3:2 - k // 3 + H, 2 - k % 3:2 - k % 3 + W] for k in range(9))

    ones = np.ones((1, 1, 9, H, W))
    cnt = np.zeros((1, 1, 9, H + 2, W + 2))
    cnt[..., 1:-1, 1:-1] = ones
    n = sum(cnt[:, :, k, 2 - k // 3:2 - k // 3 + H, 2 - k % 3:2 - k % 3 + W] for k in range(9)) * f * f
    n = np.broadcast_to(n, (B, C, H, W)).astype(np.int64)
    return ((scale * gather(T), abs(scale) * gather(Ts), abs(scale) * gather(Tsa), n),
            (gm.reshape(shape), Bm0.reshape(shape), Bm1.reshape(shape)))


def delta_grad_flow(Sg, Sga, scale):
    k0 = header_macros()["FN2U_K0_G"]
    return U23 * (k0 * Sg + Sga) + k0 * SUB * max(1.0, abs(scale))


def delta_grad_mask(exact, Bm0, Bm1, scale, dtype="float32"):
    """``dtype``: the mask's, "float32", "float16" or "bfloat16": a 16-bit gradient is the fp32 value rounded once more."""
    k0 = header_macros()["FN2U_K0_M"]
    d = U23 * (k0 * Bm0 + Bm1) + k0 * SUB * max(1.0, abs(scale))
    if dtype == "float16":
        d = d + 2.0 ** -11 * (np.abs(exact) + d) + 2.0 ** -25
    elif dtype == "bfloat16":
        d = d + 2.0 ** -8 * (np.abs(exact) + d)
    return d


def compose(flow, mask, f, scale):
    """RAFT's ``upsample_flow`` in torch, in the tensors' dtype and on their device, with ``scale`` in the place of its 8."""
    import torch
    import torch.nn.functional as F
    N, C, H, W = flow.shape
    mask = torch.softmax(mask.view(N, 1, 9, f, f, H, W), dim=2)
    up = F.unfold(scale * flow, [3, 3], padding=1).view(N, C, 9, 1, 1, H, W)
    up = torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, C, f * H, f * W)
    return up
