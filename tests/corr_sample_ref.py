"""float64 reference of CorrSample (include/preview/flownet2_hip_sample.h), written from the header's formulas term by term -- tap
by tap, corner by corner -- on top of ``corr_lookup_ref.decode``; the header's bound; and the coordinate families of
tests/test_gpu_corr_lookup.py.  Test infrastructure only.

    c = fl32(coords * 2^-l); x0 = floor(cx), fx = fl32(cx - x0)     (fp32, as the header defines it; everything after it in float64)
    out[b, l D^2 + i D + j, y, x] = sum_{ox,oy} w(ox,oy) * level_l[p, y0 + j - r + oy, x0 + i - r + ox],  p = (b H + y) W + x

Per element the functions return the exact value and S = sum |w V| (forward) or sum |gO w| (backward) over the element's terms, and
for the backward the number of terms that reach the element.  A corner outside the level is absent; a pixel whose level-0
coordinates are not finite or have |c| >= 2^20 has no taps at any level.  Levels are arrays (B H W) x H2 x W2 or (B H W) x 1 x H2 x W2.
"""
import os
import re

import numpy as np

import corr_lookup_ref as RL

SUB = 2.0 ** -149
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "preview", "flownet2_hip_sample.h")
FAMILIES = ("a", "b", "c", "d", "e2", "g")


def header_macros():
    """The integer macros of the header: FN2P_ABI_VERSION, FN2P_MAX_LEVELS, FN2P_MAX_RADIUS, FN2P_BOUND_LOG2, ..."""
    return {k: int(v) for k, v in re.findall(r"^#define (FN2P_[A-Z0-9_]+) (-?\d+)\b", open(HEADER).read(), flags=re.M)}


def bound(S):
    """|err| <= 2^FN2P_BOUND_LOG2 S + 8 * 2^-149, per element."""
    return 2.0 ** header_macros()["FN2P_BOUND_LOG2"] * np.asarray(S, dtype=np.float64) + 8 * SUB


def coords(fam, B, H, W, H2, W2, r, seed):
    """B x 2 x H x W float32 coordinates (a torch tensor) of one family of tests/test_gpu_corr_lookup.py::_coords, in cells of a
    level 0 of H2 x W2: a smooth; b integers (weight-0 taps are still terms); c border values and (-1, 0) fractions; d far
    outside; e2 uniform random; g family a with NaN, +-inf, +-1e30, +-2^20."""
    from test_gpu_corr_lookup import _coords
    assert fam in FAMILIES, fam
    return _coords(fam, B, H, W, H2, W2, r, seed)


def _level(t):
    t = np.asarray(t, dtype=np.float64)
    return t[:, 0] if t.ndim == 4 else t


def _taps(co, l, r, H2, W2):
    """Yields (k, weight (B,H,W), valid (B,H,W), yy, xx clamped) for every tap and corner of level l."""
    co = np.asarray(co, dtype=np.float32)
    ok0 = RL.decode(co)[4]
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = (co * np.float32(2.0 ** -l)).astype(np.float32)      # one fp32 multiply
    x0, y0, fx, fy, _ = RL.decode(np.where(ok0[:, None], scaled, np.float32(0)))
    D = 2 * r + 1
    for i in range(D):
        for j in range(D):
            for oy in (0, 1):
                for ox in (0, 1):
                    xx, yy = x0 + i - r + ox, y0 + j - r + oy
                    w = (fx if ox else 1.0 - fx) * (fy if oy else 1.0 - fy)
                    valid = ok0 & (xx >= 0) & (xx < W2) & (yy >= 0) & (yy < H2)
                    yield i * D + j, w, valid, np.clip(yy, 0, H2 - 1), np.clip(xx, 0, W2 - 1)


def forward(levels, co, r):
    """(exact, S), float64, B x (L D^2) x H x W."""
    B, _, H, W = np.shape(co)
    D2 = (2 * r + 1) ** 2
    out, S = np.zeros((B, len(levels) * D2, H, W)), np.zeros((B, len(levels) * D2, H, W))
    p = np.arange(B * H * W).reshape(B, H, W)
    for l, lvl in enumerate(map(_level, levels)):
        assert lvl.shape[0] == B * H * W, lvl.shape
        for k, w, valid, yy, xx in _taps(co, l, r, *lvl.shape[1:]):
            t = np.where(valid, w * lvl[p, yy, xx], 0.0)
            out[:, l * D2 + k] += t
            S[:, l * D2 + k] += np.abs(t)
    return out, S


def backward(shapes, co, gout, r):
    """[(grad, S, n)] per level, float64 (B H W) x H2 x W2: the gradient, its S and the number of terms that reach each cell.
    ``shapes``: (H2, W2) per level."""
    go = np.asarray(gout, dtype=np.float64)
    B, _, H, W = go.shape
    D2 = (2 * r + 1) ** 2
    p = np.arange(B * H * W).reshape(B, H, W)
    res = []
    for l, (H2, W2) in enumerate(shapes):
        g, S, n = np.zeros((B * H * W, H2, W2)), np.zeros((B * H * W, H2, W2)), np.zeros((B * H * W, H2, W2), dtype=np.int64)
        for k, w, valid, yy, xx in _taps(co, l, r, H2, W2):
            t = go[:, l * D2 + k] * w
            idx = (p[valid], yy[valid], xx[valid])
            np.add.at(g, idx, t[valid])
            np.add.at(S, idx, np.abs(t[valid]))
            np.add.at(n, idx, 1)
        res.append((g, S, n))
    return res


def pyramid_shapes(shape0, L):
    """RAFT's level sizes: avg_pool2d(2, 2) floors."""
    out = [tuple(shape0)]
    for _ in range(L - 1):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out
