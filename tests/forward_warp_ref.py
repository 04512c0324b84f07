"""float64 reference of ForwardWarp (include/flownet2_hip_splat.h), written from the header's formulas with numpy scatter-adds --
not from the kernels' tiling; ``compose``, the PyTorch composition (``index_put_(accumulate=True)`` over the four taps); the
header's sums emulated in numpy float32; and the flow and input families the tests share.  Test infrastructure only.

The fp32 values of fx, fy, ax, ay, bx, by are taken as the header defines them; everything after them is float64, except the
fixed-point result of the deterministic contract, which restates the fp32 contributions and sums them exactly in int64.

    fx = fl32(x + flow_x)   valid = -1 < fx < W and -1 < fy < H   x0 = floor(fx)   ax = fl32(fx - x0)   bx = fl32(1 - ax)
    out[b, c, y0 + dy, x0 + dx] += w_dydx * input[b, c, y, x]     w00 = bx by, w01 = ax by, w10 = bx ay, w11 = ax ay
"""
import os
import re

import numpy as np

U23 = 2.0 ** -23
SUB = 2.0 ** -149
TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))   # (dy, dx) in the header's order

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flownet2_hip_splat.h")


def header_macros():
    """The integer macros of the header: FN2S_ABI_VERSION, FN2S_TILE_H, FN2S_TILE_W, FN2S_HALO, FN2S_CHANNEL_GROUP, FN2S_K_I, FN2S_K_F."""
    txt = open(_HDR).read()
    return {k: int(v) for k, v in re.findall(r"^#define (FN2S_[A-Z0-9_]+) (\d+)\s*$", txt, flags=re.M)}


def taps(flow):
    """valid (B x H x W bool), x0, y0 (int64; 0 where invalid) and the fp32 values ax, ay, bx, by (0 where invalid)."""
    flow = np.asarray(flow, dtype=np.float32)
    B, _, H, W = flow.shape
    with np.errstate(invalid="ignore", over="ignore"):
        fx = (np.arange(W, dtype=np.int64).astype(np.float32)[None, None, :] + flow[:, 0]).astype(np.float32)
        fy = (np.arange(H, dtype=np.int64).astype(np.float32)[None, :, None] + flow[:, 1]).astype(np.float32)
        valid = (fx > -1) & (fx < np.float32(W)) & (fy > -1) & (fy < np.float32(H))
    fx, fy = np.where(valid, fx, np.float32(0)), np.where(valid, fy, np.float32(0))
    flx, fly = np.floor(fx), np.floor(fy)
    ax, ay = (fx - flx).astype(np.float32), (fy - fly).astype(np.float32)
    bx, by = (np.float32(1) - ax).astype(np.float32), (np.float32(1) - ay).astype(np.float32)
    zero = np.float32(0)
    return dict(valid=valid, x0=flx.astype(np.int64), y0=fly.astype(np.int64), ax=np.where(valid, ax, zero), ay=np.where(valid, ay, zero),
                bx=np.where(valid, bx, zero), by=np.where(valid, by, zero))


def _weights(t, dtype):
    ax, ay, bx, by = (t[k].astype(dtype) for k in ("ax", "ay", "bx", "by"))
    return [(bx * by).astype(dtype), (ax * by).astype(dtype), (bx * ay).astype(dtype), (ax * ay).astype(dtype)]


def _inside(t, dy, dx, H, W):
    yy, xx = t["y0"] + dy, t["x0"] + dx
    return t["valid"] & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W), yy, xx


def forward(inp, flow):
    """out, S = sum |w v| and n = the number of contributions of non-zero weight, each B x C x H x W (float64, float64, int64)."""
    inp64 = np.asarray(inp, dtype=np.float32).astype(np.float64)
    B, C, H, W = inp64.shape
    t = taps(flow)
    out, S, n = np.zeros((B, C, H, W)), np.zeros((B, C, H, W)), np.zeros((B, C, H, W), np.int64)
    for (dy, dx), w in zip(TAPS, _weights(t, np.float64)):
        m, yy, xx = _inside(t, dy, dx, H, W)
        m = m & (w != 0)
        b, y, x = np.nonzero(m)
        for c in range(C):
            v = w[b, y, x] * inp64[b, c, y, x]
            np.add.at(out[:, c], (b, yy[b, y, x], xx[b, y, x]), v)
            np.add.at(S[:, c], (b, yy[b, y, x], xx[b, y, x]), np.abs(v))
            np.add.at(n[:, c], (b, yy[b, y, x], xx[b, y, x]), 1)
    return out, S, n


def forward_bound(S, n):
    """The header's forward bound per cell."""
    return (n + 2) * U23 * S + (n + 2) * SUB


def forward_fixed(inp, flow, mutate=None):
    """The deterministic contract's result, float32 B x C x H x W, computed exactly: the fp32 contributions v = fl32(fl32(w) x),
    q = rne(v 2^s) as int64 with s = 62 - E - K per plane, exact integer sums, (float)((double)Q 2^-s).  ``mutate="float_scale"``
    plants a mistake for the tests' teeth: v 2^s formed in float32 with 2^s as a float32 of its own."""
    inp = np.asarray(inp, dtype=np.float32)
    B, C, H, W = inp.shape
    t = taps(flow)
    K = (H * W - 1).bit_length()
    out = np.zeros((B, C, H, W), np.float32)
    ws = _weights(t, np.float32)
    for b in range(B):
        for c in range(C):
            M = np.abs(inp[b, c]).max()
            if not np.isfinite(M):
                out[b, c] = np.nan
                continue
            if M == 0:
                continue
            E = int(np.frexp(np.float64(M))[1])
            s = 62 - E - K
            Q = np.zeros((H, W), np.int64)
            for (dy, dx), w in zip(TAPS, ws):
                m, yy, xx = _inside(t, dy, dx, H, W)
                y, x = np.nonzero(m[b] & (w[b] != 0))
                v = (w[b, y, x] * inp[b, c, y, x]).astype(np.float32)
                if mutate == "float_scale":
                    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                        scaled = (v * np.float32(2.0 ** s if s < 128 else np.inf)).astype(np.float32).astype(np.float64)
                    q = np.rint(np.where(np.isfinite(scaled), scaled, 0.0)).astype(np.int64)
                else:
                    q = np.rint(np.ldexp(v.astype(np.float64), s)).astype(np.int64)
                np.add.at(Q, (yy[b, y, x], xx[b, y, x]), q)
            out[b, c] = np.ldexp(Q.astype(np.float64), -s).astype(np.float32)
    return out


def backward(inp, flow, go):
    """(grad_input, Si), (grad_flow, Sf): the gradients in float64 with the magnitude sums of the header's bounds.
    Si = sum_t |w_t gO_t| (B x C x H x W); Sf = sum_c |input_c| (by (|gO01| + |gO00|) + ay (|gO11| + |gO10|)) and its y twin
    (B x 2 x H x W)."""
    inp64 = np.asarray(inp, dtype=np.float32).astype(np.float64)
    go = np.asarray(go, dtype=np.float64)
    B, C, H, W = inp64.shape
    t = taps(flow)
    w = _weights(t, np.float64)
    g = []
    for dy, dx in TAPS:
        m, yy, xx = _inside(t, dy, dx, H, W)
        yy, xx = np.where(m, yy, 0), np.where(m, xx, 0)
        bidx = np.arange(B)[:, None, None, None]
        cidx = np.arange(C)[None, :, None, None]
        g.append(np.where(m[:, None], go[bidx, cidx, yy[:, None], xx[:, None]], 0.0))
    wc = [x[:, None] for x in w]
    gi = sum(wc[k] * g[k] for k in range(4))
    Si = sum(np.abs(wc[k] * g[k]) for k in range(4))
    ax, ay, bx, by = (t[k].astype(np.float64)[:, None] for k in ("ax", "ay", "bx", "by"))
    g00, g01, g10, g11 = g
    gfx = (inp64 * (by * (g01 - g00) + ay * (g11 - g10))).sum(1)
    gfy = (inp64 * (bx * (g10 - g00) + ax * (g11 - g01))).sum(1)
    a = [np.abs(x) for x in g]
    Sfx = (np.abs(inp64) * (by * (a[1] + a[0]) + ay * (a[3] + a[2]))).sum(1)
    Sfy = (np.abs(inp64) * (bx * (a[2] + a[0]) + ax * (a[3] + a[1]))).sum(1)
    return (gi, Si), (np.stack([gfx, gfy], 1), np.stack([Sfx, Sfy], 1))


def compose(inp, flow):
    """The PyTorch composition a user writes without this layer: four ``index_put_(accumulate=True)`` over index tensors,
    differentiable in ``inp`` and ``flow`` (torch tensors of one dtype, any device)."""
    import torch
    B, C, H, W = inp.shape
    xs = torch.arange(W, device=inp.device, dtype=inp.dtype)[None, None, :]
    ys = torch.arange(H, device=inp.device, dtype=inp.dtype)[None, :, None]
    fx, fy = xs + flow[:, 0], ys + flow[:, 1]
    valid = (fx > -1) & (fx < W) & (fy > -1) & (fy < H)
    fx, fy = torch.where(valid, fx, torch.zeros_like(fx)), torch.where(valid, fy, torch.zeros_like(fy))
    x0, y0 = fx.detach().floor(), fy.detach().floor()
    ax, ay = fx - x0, fy - y0
    bx, by = 1 - ax, 1 - ay
    x0, y0 = x0.long(), y0.long()
    bidx = torch.arange(B, device=inp.device)[:, None, None].expand(B, H, W)
    out = torch.zeros(B, H, W, C, dtype=inp.dtype, device=inp.device)
    src = inp.permute(0, 2, 3, 1)
    for (dy, dx), w in zip(TAPS, (bx * by, ax * by, bx * ay, ax * ay)):
        yy, xx = y0 + dy, x0 + dx
        m = valid & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        out = out.index_put((bidx[m], yy[m], xx[m]), w[m][:, None] * src[m], accumulate=True)
    return out.permute(0, 3, 1, 2)


# ---- the flow families of the tests (seeded, float32)
def flow_family(name, B, H, W, seed=0):
    rng = np.random.default_rng(seed)
    if name == "smooth":
        f = np.array([2.25, -1.5])[None, :, None, None] + 0.3 * rng.standard_normal((B, 2, H, W))
    elif name == "random":
        f = rng.uniform(-1.5, 1.5, (B, 2, H, W)) * np.array([W, H])[None, :, None, None]
    elif name == "converge":
        f = np.empty((B, 2, H, W))
        f[:, 0] = (W // 2 + 0.5) - np.arange(W)[None, None, :]
        f[:, 1] = (H // 2 + 0.25) - np.arange(H)[None, :, None]
    elif name == "zero":
        f = np.zeros((B, 2, H, W))
    elif name == "shift":
        f = np.empty((B, 2, H, W))
        f[:, 0], f[:, 1] = 3.0, -2.0
    else:
        raise ValueError(name)
    return f.astype(np.float32)


def inside_share(flow):
    """The share of the 4 H W B taps that lie inside the image."""
    B, _, H, W = flow.shape
    t = taps(flow)
    return sum(_inside(t, dy, dx, H, W)[0].sum() for dy, dx in TAPS) / (4.0 * B * H * W)


# ---- the input families of the tests (seeded, float32)
INPUT_FAMILIES = ("normal", "graded", "cancel", "subnormal", "huge")
GRADED_EXPONENTS = (-100, -20, 0, 20, 100)
# the flows each input family is combined with: a plane maximum of 2^126 cannot take the converge flow's H W terms in one cell
FAMILY_FLOWS = {"normal": ("smooth", "converge", "shift"), "graded": ("smooth", "converge", "shift"), "cancel": ("smooth", "converge", "shift"),
                "subnormal": ("smooth", "converge", "shift"), "huge": ("smooth", "zero", "shift")}


def input_family(name, shape, seed):
    """(input, grad_out), float32 B x C x H x W each.  Each family asserts on its own output -- with the flows of ``flow_family``
    it is meant for -- that it still does what it is for:
      normal     standard normal, both
      graded     plane (b, c) scaled by 2^e, e cycling through GRADED_EXPONENTS with b C + c; grad_out standard normal / 8 scaled
                 by 2^-e: every product of the gradients stays below 2^100
      cancel     signs alternate from source pixel to source pixel, magnitudes in [1, 1 + 2^-10]: under ``converge`` the cells
                 that receive everything hold |sum| <= 2^-6 sum |w v|
      subnormal  planes alternate between |v| in (0, 2^-127] and |v| in [2^-125, 2^-120]: every value of the first kind is
                 subnormal, and under ``smooth`` at least 10 % of the second kind's contributions are
      huge       every plane's maximum in [2^125, 2^126): under ``smooth``, ``zero`` and ``shift`` every cell's sum |w v| stays
                 below 2^127, so no partial sum in any order overflows"""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    inp = rng.standard_normal(shape)
    go = rng.standard_normal(shape)
    plane = (np.arange(B)[:, None] * C + np.arange(C)[None, :])[:, :, None, None]
    if name == "normal":
        pass
    elif name == "graded":
        e = np.array(GRADED_EXPONENTS, np.float64)[plane % len(GRADED_EXPONENTS)]
        inp, go = inp * 2.0 ** e, go / 8 * 2.0 ** -e
        assert np.abs(inp).max() < 2.0 ** 103 and np.abs(go).max() < 2.0 ** 100 and np.abs(inp * go).max() < 2.0 ** 100
        assert (np.abs(inp).max(axis=(2, 3)) * np.abs(go).max(axis=(2, 3))).max() * C < 2.0 ** 100
    elif name == "cancel":
        sign = 1.0 - 2.0 * (np.arange(H * W).reshape(H, W) % 2)
        inp = sign * (1 + 2.0 ** -10 * rng.random(shape))
    elif name == "subnormal":
        tiny = 2.0 ** -127 * (2.0 ** -22 + (1 - 2.0 ** -22) * rng.random(shape)) * np.sign(inp)
        small = 2.0 ** (-125 + 5 * rng.random(shape)) * np.sign(inp)
        inp = np.where(plane % 2 == 0, tiny, small)
    elif name == "huge":
        inp = inp / np.abs(inp).max(axis=(2, 3), keepdims=True) * 2.0 ** 125 * (1 + rng.random((B, C, 1, 1)) * (1 - 2.0 ** -20))
    else:
        raise ValueError(name)
    inp, go = inp.astype(np.float32), go.astype(np.float32)
    assert np.isfinite(inp).all() and np.isfinite(go).all()
    if H * W >= 17 * 67:
        if name == "cancel":
            out, S, n = forward(inp, flow_family("converge", B, H, W))
            full = n == H * W
            assert full.any() and (np.abs(out[full]) <= 2.0 ** -6 * S[full]).all()
        if name == "subnormal":
            a = np.abs(inp.astype(np.float64))
            first = np.broadcast_to(plane % 2 == 0, shape)
            assert (a[first] > 0).all() and (a[first] <= 2.0 ** -127).all() and (a[~first] >= 2.0 ** -125).all() and (a[~first] <= 2.0 ** -120).all()
            t = taps(flow_family("smooth", B, H, W))
            below = total = 0
            for (dy, dx), w in zip(TAPS, _weights(t, np.float64)):
                m = _inside(t, dy, dx, H, W)[0] & (w != 0)
                v = np.abs(w[:, None] * a)[np.broadcast_to(m[:, None], shape) & ~first]
                below, total = below + (v < 2.0 ** -126).sum(), total + v.size
            assert below >= 0.1 * total, (below, total)
        if name == "huge":
            top = np.abs(inp.astype(np.float64)).max(axis=(2, 3))
            assert (top >= 2.0 ** 125).all() and (top < 2.0 ** 126).all()
            for fl in FAMILY_FLOWS["huge"]:
                assert forward(inp, flow_family(fl, B, H, W))[1].max() < 2.0 ** 127
    return inp, go


# ---- the header's operation list in float32
def emulate_forward(inp, flow, mutate=None):
    """The atomic forward in numpy float32: every contribution fl32(fl32(w) x) added to its cell in float32, one rounding per
    addition, in the order of the source pixels, tap by tap -- one of the orders the atomics may take.  ``mutate="ftz_add"``
    plants a mistake: an addition whose result is subnormal gives 0."""
    inp = np.asarray(inp, np.float32)
    B, C, H, W = inp.shape
    t = taps(flow)
    out = np.zeros((B, C, H, W), np.float32)
    tiny = np.float32(2.0 ** -126)
    with np.errstate(under="ignore"):
        for (dy, dx), w in zip(TAPS, _weights(t, np.float32)):
            m, yy, xx = _inside(t, dy, dx, H, W)
            b, y, x = np.nonzero(m & (w != 0))
            for c in range(C):
                v = (w[b, y, x] * inp[b, c, y, x]).astype(np.float32)
                if mutate == "ftz_add":
                    for i in range(v.size):
                        s = np.float32(out[b[i], c, yy[b[i], y[i], x[i]], xx[b[i], y[i], x[i]]] + v[i])
                        out[b[i], c, yy[b[i], y[i], x[i]], xx[b[i], y[i], x[i]]] = s if abs(s) >= tiny else np.float32(0)
                else:
                    np.add.at(out[:, c], (b, yy[b, y, x], xx[b, y, x]), v)
    return out


def emulate_backward(inp, flow, go):
    """(grad_input, grad_flow) in numpy float32, the header's sums operation by operation: every sum from +0, one rounding per
    operation, taps in the order 00, 01, 10, 11, channels ascending."""
    f32 = np.float32
    inp, go = np.asarray(inp, f32), np.asarray(go, f32)
    B, C, H, W = inp.shape
    t = taps(flow)
    g = []
    bidx, cidx = np.arange(B)[:, None, None, None], np.arange(C)[None, :, None, None]
    for dy, dx in TAPS:
        m, yy, xx = _inside(t, dy, dx, H, W)
        yy, xx = np.where(m, yy, 0), np.where(m, xx, 0)
        g.append(np.where(m[:, None], go[bidx, cidx, yy[:, None], xx[:, None]], f32(0)))
    with np.errstate(under="ignore"):
        w = [x[:, None] for x in _weights(t, f32)]
        gi = np.zeros((B, C, H, W), f32)
        for k in range(4):
            gi = gi + w[k] * g[k]
        ax, ay, bx, by = (t[k][:, None] for k in ("ax", "ay", "bx", "by"))
        g00, g01, g10, g11 = g
        tx = inp * (by * (g01 - g00) + ay * (g11 - g10))
        ty = inp * (bx * (g10 - g00) + ax * (g11 - g01))
        gfx, gfy = np.zeros((B, H, W), f32), np.zeros((B, H, W), f32)
        for c in range(C):
            gfx, gfy = gfx + tx[:, c], gfy + ty[:, c]
    return gi, np.stack([gfx, gfy], 1)


def fixed_bound(inp, S, n):
    """What the header promises of the deterministic forward: the forward bound plus 2^(K - 62) M per contribution."""
    inp = np.asarray(inp, np.float32)
    H, W = inp.shape[2:]
    K = (H * W - 1).bit_length()
    M = np.abs(inp.astype(np.float64)).max(axis=(2, 3), keepdims=True)
    return forward_bound(S, n) + n * 2.0 ** (K - 62) * M
