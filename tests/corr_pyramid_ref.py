"""float64 reference of CorrPyramid (include/preview/flownet2_hip_pyramid.h), written from the header's formulas; the header's bound;
and float32 restatements of the pooling order and of the fold for the bit-exact checks.  Test infrastructure only.

    level 0      v0[p, v, u] = s sum_c fmap1[b, c, y, x] fmap2[b, c, v, u],  p = (b H + y) W + x,  s = 1 / sqrt(C)
    level l + 1  the mean of the 2 x 2 block of level l; sizes H2 >> l x W2 >> l (a ragged last row or column is dropped)
    G[p, v, u]   s (g0 + 1/4 g1[v>>1, u>>1] + 1/16 g2[v>>2, u>>2] + 1/64 g3[v>>3, u>>3]), a term absent outside its level
    grad_fmap1[b, c, p] = sum_q G[p, q] fmap2[b, c, q],   grad_fmap2[b, c, q] = sum_p G[p, q] fmap1[b, c, p]

Everything is a torch tensor; levels and their gradients are (B H W) x H2_l x W2_l.  ``mutation`` names one deliberate mistake, for
the tests that show the bound notices it.
"""
import math
import os
import re

import torch

import corr_contract_ref as CR

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "preview", "flownet2_hip_pyramid.h")
U23 = 2.0 ** -23
MUTATIONS = ("scale", "ceil", "swap", "pool_half", "fold_weight")
# (B, C, (H, W), (H2, W2), L): the shapes of tests/test_gpu_corr_pyramid.py
SHAPES = [(2, 40, (9, 11), (9, 11), 2), (1, 256, (21, 28), (21, 28), 4), (2, 32, (8, 16), (17, 35), 4), (1, 8, (3, 5), (8, 8), 1),
          (2, 64, (16, 32), (16, 32), 4)]


def shape_id(s):
    return "%dx%dx%dx%d-%dx%d-L%d" % (s[0], s[1], *s[2], *s[3], s[4])


def header_macros():
    """The macros of the header as Python numbers (the bound's are C hexadecimal float expressions)."""
    out = {}
    for k, v in re.findall(r"^#define (FN2Y_[A-Z0-9_]+) (.+?)\s*(?:/\*.*)?$", open(HEADER).read(), flags=re.M):
        v = re.sub(r"0x1p(-?\d+)", lambda m: "2.0 ** %s" % m.group(1), v)
        out[k] = eval(v, {"__builtins__": {}})   # arithmetic on literals only
    return out


def inputs(shape, seed):
    """fmap1, fmap2: N(0, 1), float32."""
    B, C, (H, W), (H2, W2), _ = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H2, W2, generator=g)


def level_sizes(H2, W2, L, ceil=False):
    sizes = [(H2, W2)]
    for _ in range(L - 1):
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2) if ceil else (h // 2, w // 2))
    return sizes


def pool_exact(x, ceil=False, weight=0.25):
    """The mean over the 2 x 2 blocks of (P, h, w); a ragged last row or column is dropped (``ceil``: kept, averaged over what is there)."""
    if ceil:
        return torch.nn.functional.avg_pool2d(x[:, None], 2, stride=2, ceil_mode=True)[:, 0]
    h, w = x.shape[-2] // 2, x.shape[-1] // 2
    a, b = x[:, 0:2 * h:2, 0:2 * w:2], x[:, 0:2 * h:2, 1:2 * w:2]
    c, d = x[:, 1:2 * h:2, 0:2 * w:2], x[:, 1:2 * h:2, 1:2 * w:2]
    return ((a + b) + (c + d)) * weight


def forward(fmap1, fmap2, L, mutation=None):
    """(levels, S0): the float64 levels of the float32 maps and S0 = s sum_c |fmap1 fmap2| per element of level 0."""
    if mutation == "swap":
        fmap1, fmap2 = fmap2, fmap1
    B, C, H, W = fmap1.shape
    H2, W2 = fmap2.shape[2:]
    a, b = fmap1.double().reshape(B, C, H * W), fmap2.double().reshape(B, C, H2 * W2)
    s = 1.0 / C if mutation == "scale" else 1.0 / math.sqrt(C)
    v0 = (s * torch.einsum("bcp,bcq->bpq", a, b)).reshape(B * H * W, H2, W2)
    S0 = (s * torch.einsum("bcp,bcq->bpq", a.abs(), b.abs())).reshape(B * H * W, H2, W2)
    levels = [v0]
    for l in range(1, L):
        levels.append(pool_exact(levels[-1], ceil=mutation == "ceil", weight=0.5 if mutation == "pool_half" and l == L - 1 else 0.25))
    return levels, S0


def bounds(levels, S0, C):
    """delta_l of the header, per element of each level: delta_0 is corr_contract_ref.delta_bf16x3 with n = C, delta_l = pool_l(delta_0) +
    l FN2Y_BOUND_PER_POOL pool_l(S0)."""
    m = header_macros()
    assert m["FN2Y_BOUND_SPLIT"] == 2 * 2.0 ** -24 + 2.0 ** -32 and m["FN2Y_BOUND_PER_CHANNEL"] == 6 * U23 * (1 + 2.0 ** -7)
    d, S = CR.delta_bf16x3(levels[0], S0, C), S0
    out = [d]
    for l in range(1, len(levels)):
        d, S = pool_exact(d), pool_exact(S)
        out.append(d + l * m["FN2Y_BOUND_PER_POOL"] * S)
    return out


def fold(grads, C, H2, W2, mutation=None):
    """G (P, H2, W2) in the dtype of the gradients (float64 here) from the levels' gradients; None is a missing one."""
    first = next(g for g in grads if g is not None)
    G = torch.zeros((first.shape[0], H2, W2), dtype=first.dtype)
    for l, g in enumerate(grads):
        if g is None:
            continue
        g = g.reshape(g.shape[0], H2 >> l, W2 >> l)
        w = 0.125 if mutation == "fold_weight" and l == 2 else 0.25 ** l
        up = g.repeat_interleave(2 ** l, dim=1).repeat_interleave(2 ** l, dim=2)
        G[:, :up.shape[1], :up.shape[2]] += w * up
    return G / math.sqrt(C)


def backward(fmap1, fmap2, grads, mutation=None):
    """(G, grad_fmap1, grad_fmap2) in float64."""
    B, C, H, W = fmap1.shape
    H2, W2 = fmap2.shape[2:]
    G = fold([None if g is None else g.double() for g in grads], C, H2, W2, mutation)
    Gb = G.reshape(B, H * W, H2 * W2)
    g1 = torch.einsum("bpq,bcq->bcp", Gb, fmap2.double().reshape(B, C, -1)).reshape(fmap1.shape)
    g2 = torch.einsum("bpq,bcp->bcq", Gb, fmap1.double().reshape(B, C, -1)).reshape(fmap2.shape)
    return G, g1, g2


def composition(fmap1, fmap2, L):
    """RAFT's CorrBlock.__init__ in the dtype of the maps: matmul / sqrt(C), avg_pool2d; levels (B H W) x 1 x H2_l x W2_l."""
    B, C, H, W = fmap1.shape
    corr = torch.matmul(fmap1.reshape(B, C, H * W).transpose(1, 2), fmap2.reshape(B, C, -1)) / math.sqrt(C)
    pyr = [corr.reshape(B * H * W, 1, *fmap2.shape[2:])]
    for _ in range(L - 1):
        pyr.append(torch.nn.functional.avg_pool2d(pyr[-1], 2, stride=2))
    return pyr


# ---- float32 restatements (CPU tensors: IEEE adds, no flushing)
def pool32(level):
    """The next level from a float32 level (P, h, w): fl32(((a + b) + (c + d)) * 0.25f), every add rounded on its own."""
    assert level.dtype == torch.float32 and level.device.type == "cpu"
    return pool_exact(level)


def fold32(grads, C, H2, W2):
    """G from float32 gradients in the header's order: the sum starts from g0 (+0 where it is missing), one rounded add per level
    present, only where the level reaches; then the product with s = fl32(1 / sqrt(C))."""
    first = next(g for g in grads if g is not None)
    assert first.dtype == torch.float32 and first.device.type == "cpu"
    P = first.shape[0]
    acc = torch.zeros((P, H2, W2), dtype=torch.float32) if grads[0] is None else grads[0].reshape(P, H2, W2).clone()
    for l in range(1, len(grads)):
        if grads[l] is None:
            continue
        g = grads[l].reshape(P, H2 >> l, W2 >> l)
        up = (torch.tensor(0.25 ** l, dtype=torch.float32) * g).repeat_interleave(2 ** l, dim=1).repeat_interleave(2 ** l, dim=2)
        h, w = up.shape[1:]
        acc[:, :h, :w] = acc[:, :h, :w] + up
    s = torch.tensor(1.0 / math.sqrt(C), dtype=torch.float64).to(torch.float32)
    return s * acc


def misses(got, want, deltas):
    """Whether ``got`` (levels) misses the bound around ``want`` somewhere: a level of another shape, or an element outside delta."""
    if len(got) != len(want):
        return True
    for g, w, d in zip(got, want, deltas):
        g = g.reshape(g.shape[0], *g.shape[-2:])
        if g.shape != w.shape or bool(((g.double() - w).abs() > d).any()):
            return True
    return False


def worst_ratio(got, want, deltas):
    """max |got - want| / delta over all levels, and per level."""
    per = [float(((g.reshape(w.shape).double() - w).abs() / d).max()) for g, w, d in zip(got, want, deltas)]
    return max(per), per
