"""float64 reference of CorrSample1d (include/staging/flownet2_hip_sample1d.h), written from the header's formulas term by term; the
header's bound and macros; the coordinate families of the tests; RAFT-Stereo's composition (CorrBlock1D, ``reg``) in any dtype.
Test infrastructure only; no test functions.

    c = fl32(coords_x * 2^-l); x0 = floor(c), fx = fl32(c - x0)     (fp32, as the header defines it; everything after it in float64)
    out[b, l D + i, y, x] = (1 - fx) * level_l[p, x0 + i - r] + fx * level_l[p, x0 + i - r + 1],  p = (b H + y) W + x

Per element the functions return the exact value and S = sum |w V| (forward) or sum |gO w| (backward) over the element's terms, and
for the backward the number of terms that reach the element.  A cell outside the level is absent; a pixel whose level-0 coordinate
is not finite or has |c| >= 2^20 has no taps at any level.  Levels are arrays (B H W) x W2 or (B H W) x 1 x 1 x W2; coordinates are
B x 1 x H x W or B x 2 x H x W, of which channel 0 is read.
"""
import os
import re

import numpy as np

SUB = 2.0 ** -149
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "staging", "flownet2_hip_sample1d.h")
FAMILIES = ("a", "b", "c", "d", "e", "g")


def header_macros():
    """The integer macros of the header: FN2H_ABI_VERSION, FN2H_MAX_LEVELS, FN2H_MAX_RADIUS, FN2H_BOUND_LOG2, ..."""
    return {k: int(v) for k, v in re.findall(r"^#define (FN2H_[A-Z0-9_]+) (-?\d+)\b", open(HEADER).read(), flags=re.M)}


def bound(S):
    """|err| <= 2^FN2H_BOUND_LOG2 S + 4 * 2^-149, per element."""
    return 2.0 ** header_macros()["FN2H_BOUND_LOG2"] * np.asarray(S, dtype=np.float64) + 4 * SUB


def has_taps(cx):
    """B x H x W bool: the level-0 coordinate is finite and |c| < 2^20."""
    c = np.asarray(cx, dtype=np.float32)[:, 0]
    with np.errstate(invalid="ignore"):
        return np.isfinite(c) & (np.abs(c) < np.float32(2.0 ** 20))


def decode(cx, l):
    """(x0 int64, fx float64 holding the fp32 value, ok) of level l, each B x H x W; x0 = 0, fx = 0 where not ok."""
    c = np.asarray(cx, dtype=np.float32)[:, 0]
    ok = has_taps(cx)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = (np.where(ok, c, np.float32(0)) * np.float32(2.0 ** -l)).astype(np.float32)      # one fp32 multiply
    fl = np.floor(scaled)
    fx = (scaled - fl).astype(np.float32)                                                         # the fp32 difference
    assert fx.dtype == np.float32 and scaled.dtype == np.float32
    return fl.astype(np.int64), fx.astype(np.float64), ok


def _level(t):
    t = np.asarray(t, dtype=np.float64)
    assert t.ndim == 2 or (t.ndim == 4 and t.shape[1:3] == (1, 1)), t.shape
    return t.reshape(t.shape[0], t.shape[-1])


def _taps(cx, l, r, W2):
    """Yields (i, weight (B,H,W), valid (B,H,W), xx clamped) for every tap i and both of its cells, in the header's order."""
    x0, fx, ok = decode(cx, l)
    for i in range(2 * r + 1):
        for ox in (0, 1):
            xx = x0 + i - r + ox
            w = fx if ox else 1.0 - fx
            yield i, w, ok & (xx >= 0) & (xx < W2), np.clip(xx, 0, W2 - 1)


def forward(levels, cx, r):
    """(exact, S), float64, B x (L D) x H x W."""
    B, _, H, W = np.shape(cx)
    D = 2 * r + 1
    out, S = np.zeros((B, len(levels) * D, H, W)), np.zeros((B, len(levels) * D, H, W))
    p = np.arange(B * H * W).reshape(B, H, W)
    for l, lvl in enumerate(map(_level, levels)):
        assert lvl.shape[0] == B * H * W, lvl.shape
        for i, w, valid, xx in _taps(cx, l, r, lvl.shape[1]):
            t = np.where(valid, w * lvl[p, xx], 0.0)
            out[:, l * D + i] += t
            S[:, l * D + i] += np.abs(t)
    return out, S


def backward(widths, cx, gout, r):
    """[(grad, S, n)] per level, float64 (B H W) x W2: the gradient, its S and the number of terms that reach each cell."""
    go = np.asarray(gout, dtype=np.float64)
    B, _, H, W = go.shape
    D = 2 * r + 1
    p = np.arange(B * H * W).reshape(B, H, W)
    res = []
    for l, W2 in enumerate(widths):
        g, S, n = np.zeros((B * H * W, W2)), np.zeros((B * H * W, W2)), np.zeros((B * H * W, W2), dtype=np.int64)
        for i, w, valid, xx in _taps(cx, l, r, W2):
            t = go[:, l * D + i] * w
            idx = (p[valid], xx[valid])
            np.add.at(g, idx, t[valid])
            np.add.at(S, idx, np.abs(t[valid]))
            np.add.at(n, idx, 1)
        res.append((g, S, n))
    return res


def coords(fam, B, H, W, W2, r, seed):
    """B x 1 x H x W float32 x coordinates (a torch tensor), in cells of a level 0 of W2 cells:
    a  smooth disparity, fractional, inside the level;
    b  exact integers from -r - 2 to W2 + r + 1 (weight-0 taps are still terms);
    c  -1 < c < 0 (fx rounded once), and windows that straddle either end of the level by a fraction of a cell;
    d  wholly outside, on either side;
    e  uniform random over the level and a margin of r + 2 cells;
    g  family a with NaN, +-inf, +-1e30 and +-2^20 at some pixels: no taps there."""
    import torch
    assert fam in FAMILIES, fam
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = rng.uniform(0, 6.28, (B, 1, 1))
    a = xs[None] * (W2 / W) * 0.9 + 0.37 + 0.45 * max(W2 - 1, 0) * 0.1 * (1 + np.sin(0.23 * xs[None] + 0.31 * ys[None] + ph))
    a = np.clip(a, 0.0, max(W2 - 1, 0) + 0.49)
    if fam == "a":
        c = a
    elif fam == "b":
        c = rng.integers(-r - 2, W2 + r + 2, (B, H, W)).astype(np.float64)
    elif fam == "c":
        vals = np.array([-2.0 ** -12, -2.0 ** -30, -0.3, -1 + 2.0 ** -20, -(r + 1) - 2.0 ** -10, -(r + 1) + 2.0 ** -10, -r - 0.5, -0.5 * r - 0.25,
                         W2 - 1 + r + 2.0 ** -10, W2 - 1 + r - 2.0 ** -10, W2 - 0.7, W2 - 1 - 0.5 * r + 0.25, 0.4])
        c = vals[rng.integers(0, len(vals), (B, H, W))]
    elif fam == "d":
        c = np.where(rng.random((B, H, W)) < 0.5, -100.0 - 8 * rng.random((B, H, W)), W2 + 100.0 + 8 * rng.random((B, H, W)))
    elif fam == "e":
        c = rng.uniform(-r - 2, W2 + r + 2, (B, H, W))
    else:
        c = a.copy()
        bad = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 20, -(2.0 ** 20)]
        n = min(max(int(0.1 * B * H * W), 1), 2 * len(bad))
        for k, p in enumerate(rng.choice(B * H * W, n, replace=False)):
            c[np.unravel_index(p, (B, H, W))] = bad[k % len(bad)]
    return torch.from_numpy(np.ascontiguousarray(c[:, None]).astype(np.float32))


def pyramid_widths(W2, L):
    """RAFT-Stereo's level widths: avg_pool2d([1, 2], [1, 2]) floors."""
    return [W2 >> l for l in range(L)]


# ------------------------------------------------------------------ RAFT-Stereo's composition (core/corr.py, CorrBlock1D, "reg")
def compose_lookup(pyramid, coords, r):
    """CorrBlock1D.__call__ on a prebuilt pyramid of (B H W1, 1, 1, W2_l) torch levels with W2_l >= 2, in their dtype: per level
    linspace, add, zeros_like, cat, grid_sample (bilinear, align_corners, zero padding), view; then cat, permute, contiguous.
    ``coords``: B x 2 x H x W or B x 1 x H x W, channel 0 = x."""
    import torch
    import torch.nn.functional as F
    cx = coords[:, :1].permute(0, 2, 3, 1)
    B, H, W, _ = cx.shape
    outs = []
    for l, corr in enumerate(pyramid):
        dx = torch.linspace(-r, r, 2 * r + 1, dtype=cx.dtype, device=cx.device).view(2 * r + 1, 1)
        x0 = dx + cx.reshape(B * H * W, 1, 1, 1) / 2 ** l
        y0 = torch.zeros_like(x0)
        W2 = corr.shape[-1]
        grid = torch.cat([2 * x0 / (W2 - 1) - 1, y0], dim=-1)        # bilinear_sampler: H == 1, so ygrid passes through untouched
        outs.append(F.grid_sample(corr, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(B, H, W, -1))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def compose_pyramid(fmap1, fmap2, L):
    """CorrBlock1D.corr and the pooling, in the maps' dtype."""
    import torch
    import torch.nn.functional as F
    B, C, H, W1 = fmap1.shape
    corr = torch.einsum("aijk,aijh->ajkh", fmap1, fmap2).reshape(B * H * W1, 1, 1, fmap2.shape[3]) / float(C) ** 0.5
    pyr = [corr]
    for _ in range(L - 1):
        pyr.append(F.avg_pool2d(pyr[-1], [1, 2], stride=[1, 2]))
    return pyr


def compose(fmap1, fmap2, coords, L, r):
    return compose_lookup(compose_pyramid(fmap1, fmap2, L), coords, r)
