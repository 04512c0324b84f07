"""float64 reference of CorrLookup (include/flownet2_hip_lookup.h), written from the header's formula term by term -- tap by tap,
corner by corner -- not from the kernels' grid organisation; and ``compose``, RAFT's all-pairs volume + ``grid_sample``
composition in torch.  Test infrastructure only.

    x0 = floor(cx), fx = fl32(cx - x0)        (the fp32 difference, as the header defines it; everything after it in float64)
    out[b, i D + j, y, x] = scale * sum_{ox,oy} w(ox,oy) * sum_c fmap1[b,c,y,x] * fmap2[b,c, y0 + j - r + oy, x0 + i - r + ox]

Per element the functions return the exact value, S = |scale| * sum |w a b| over the element's terms and, for grad_fmap2, the
number of terms (pixel, tap, corner) that reach it.  A tap outside fmap2 is absent; a pixel whose coordinates are not finite
or have |c| >= 2^20 has no taps.
"""
import os
import re

import numpy as np

U23 = 2.0 ** -23
SUB = 2.0 ** -149

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flownet2_hip_lookup.h")


def header_macros():
    """The integer macros of the header: FN2L_TILE_W, FN2L_PATCH_W, FN2L_STAGED_MAX_RADIUS, FN2L_K0_GRAD2, ..."""
    txt = open(_HDR).read()
    return {k: int(v) for k, v in re.findall(r"^#define (FN2L_[A-Z0-9_]+) (\d+)\s*$", txt, flags=re.M)}


def _header_expr(name, arg):
    """FN2L_K_FORWARD(C) / FN2L_K_GRAD1(r) as Python functions, from the header's text (integer expressions in one argument)."""
    m = re.search(r"^#define %s\((\w+)\) (.+)$" % name, open(_HDR).read(), flags=re.M)
    expr = m.group(2).replace("(%s)" % m.group(1), "(%d)" % arg)
    assert re.fullmatch(r"[0-9+\-*() ]+", expr), expr
    return int(eval(expr))


def k_forward(C):
    return _header_expr("FN2L_K_FORWARD", C)


def k_grad1(r):
    return _header_expr("FN2L_K_GRAD1", r)


def delta_forward(exact, S, C, scale):
    return k_forward(C) * U23 * S + U23 * np.abs(exact) + k_forward(C) * SUB * max(1.0, abs(scale))


def delta_grad1(exact, S, r, scale):
    return k_grad1(r) * U23 * S + U23 * np.abs(exact) + k_grad1(r) * SUB * max(1.0, abs(scale))


def delta_grad2(exact, S, n, scale):
    k = n + header_macros()["FN2L_K0_GRAD2"]
    return k * U23 * S + U23 * np.abs(exact) + k * SUB * max(1.0, abs(scale))


def decode(coords):
    """(x0, y0, fx, fy, ok) of B x 2 x H x W fp32 coordinates: integer floors, the fp32 fractions as float64, and the pixels
    that have taps."""
    c = np.asarray(coords, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(c[:, 0]) < np.float32(2.0 ** 20)) & (np.abs(c[:, 1]) < np.float32(2.0 ** 20))
    safe = np.where(ok[:, None], c, np.float32(0))
    fl = np.floor(safe)
    frac = (safe - fl).astype(np.float32)          # the fp32 subtraction
    return fl[:, 0].astype(np.int64), fl[:, 1].astype(np.int64), frac[:, 0].astype(np.float64), frac[:, 1].astype(np.float64), ok


def _taps(coords, r, H2, W2):
    """Yields (k, weight (B,H,W), valid (B,H,W), yy, xx clamped) for every tap and corner."""
    x0, y0, fx, fy, ok = decode(coords)
    D = 2 * r + 1
    for i in range(D):
        for j in range(D):
            for oy in (0, 1):
                for ox in (0, 1):
                    xx, yy = x0 + i - r + ox, y0 + j - r + oy
                    w = (fx if ox else 1.0 - fx) * (fy if oy else 1.0 - fy)
                    valid = ok & (xx >= 0) & (xx < W2) & (yy >= 0) & (yy < H2)
                    yield i * D + j, w, valid, np.clip(yy, 0, H2 - 1), np.clip(xx, 0, W2 - 1)


def forward(fmap1, fmap2, coords, r, scale):
    """(exact, S), float64, B x D^2 x H x W."""
    f1, f2 = np.asarray(fmap1, dtype=np.float64), np.asarray(fmap2, dtype=np.float64)
    B, C, H, W = f1.shape
    H2, W2 = f2.shape[2:]
    D = 2 * r + 1
    out, S = np.zeros((B, D * D, H, W)), np.zeros((B, D * D, H, W))
    bi = np.arange(B)[:, None, None]
    a = f1.transpose(0, 2, 3, 1)                              # B, H, W, C
    for k, w, valid, yy, xx in _taps(coords, r, H2, W2):
        prod = a * f2[bi, :, yy, xx]                          # B, H, W, C
        out[:, k] += np.where(valid, w * prod.sum(-1), 0.0)
        S[:, k] += np.where(valid, np.abs(w) * np.abs(prod).sum(-1), 0.0)
    return scale * out, abs(scale) * S


def backward(fmap1, fmap2, coords, gout, r, scale):
    """((g1, S1), (g2, S2, n2)): float64 gradients, their S, and the number of terms that reach each grad_fmap2 element."""
    f1, f2, go = (np.asarray(t, dtype=np.float64) for t in (fmap1, fmap2, gout))
    B, C, H, W = f1.shape
    H2, W2 = f2.shape[2:]
    g1, S1 = np.zeros((B, H, W, C)), np.zeros((B, H, W, C))
    g2, S2, n2 = np.zeros((B, H2, W2, C)), np.zeros((B, H2, W2, C)), np.zeros((B, H2, W2), dtype=np.int64)
    bi = np.broadcast_to(np.arange(B)[:, None, None], (B, H, W))
    a = f1.transpose(0, 2, 3, 1)
    for k, w, valid, yy, xx in _taps(coords, r, H2, W2):
        gw = np.where(valid, go[:, k] * w, 0.0)[..., None]    # B, H, W, 1
        t1 = gw * f2[bi, :, yy, xx]
        g1 += t1
        S1 += np.abs(t1)
        t2 = gw * a
        sel = valid
        np.add.at(g2, (bi[sel], yy[sel], xx[sel]), t2[sel])
        np.add.at(S2, (bi[sel], yy[sel], xx[sel]), np.abs(t2[sel]))
        np.add.at(n2, (bi[sel], yy[sel], xx[sel]), 1)
    tr = lambda t: np.ascontiguousarray(t.transpose(0, 3, 1, 2))
    n2c = np.ascontiguousarray(np.broadcast_to(n2[:, None], (B, C, H2, W2)))
    return (scale * tr(g1), abs(scale) * tr(S1)), (scale * tr(g2), abs(scale) * tr(S2), n2c)


def compose(fmap1, fmap2, coords, r, scale, num_levels=1):
    """RAFT's CorrBlock in torch, in the tensors' dtype and on their device: the all-pairs volume fmap1^T fmap2 * scale, pooled
    with avg_pool2d(2, 2) per further level, sampled by grid_sample(align_corners=True, zero padding) at coords / 2**level +
    delta, delta = stack(meshgrid(dy, dx)) added to (x, y).  B x (num_levels D^2) x H x W.  Needs H2, W2 >= 2 at every level
    (the normalisation divides by W2 - 1).  Differentiable in fmap1 and fmap2."""
    import torch
    import torch.nn.functional as F
    B, C, H, W = fmap1.shape
    H2, W2 = fmap2.shape[2:]
    D = 2 * r + 1
    corr = torch.matmul(fmap1.reshape(B, C, H * W).transpose(1, 2), fmap2.reshape(B, C, H2 * W2)) * scale
    corr = corr.reshape(B * H * W, 1, H2, W2)
    d = torch.linspace(-r, r, D, dtype=fmap1.dtype, device=fmap1.device)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, D, D, 2)
    centroid = coords.to(fmap1.dtype).permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
    outs = []
    for lvl in range(num_levels):
        if lvl:
            corr = F.avg_pool2d(corr, 2, stride=2)
        h2, w2 = corr.shape[-2:]
        assert h2 >= 2 and w2 >= 2, (h2, w2)
        xy = centroid / 2 ** lvl + delta
        grid = torch.stack((2 * xy[..., 0] / (w2 - 1) - 1, 2 * xy[..., 1] / (h2 - 1) - 1), dim=-1)
        s = F.grid_sample(corr, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        outs.append(s.view(B, H, W, D * D).permute(0, 3, 1, 2))
    return torch.cat(outs, dim=1)
