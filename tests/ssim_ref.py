"""Reference of the structural-similarity distance (include/staging/flownet2_hip_ssim.h), for the tests.  No test functions.

``compose`` is the PyTorch composition the layer replaces, written from the formula in any dtype: five ``avg_pool2d`` over x, y, x^2,
y^2, xy, the raw-moment variances, the quotient, the clamp; ``border="zero"`` embeds the valid-only result (ARFlow's ``SSIM``) in a
ring of zeros, ``border="reflect"`` pads both images with ``ReflectionPad2d(md)`` first (monodepth2's ``SSIM`` module).

``reference`` is the float64 evaluation in the header's own form -- moments about the mean, the gradient as the gather over
windows of ``Mx + A (x_q - mx) + B (y_q - my)`` and, under reflect, the adjoint of the padding -- together with the header's
per-element bounds, evaluated from float64 quantities alone.  tests/test_ssim_host.py holds its gradient to autograd of ``compose``.

``inputs`` makes the four families: (a) noise, (b) smooth images half a pixel apart, (c) identical images, (d) family (a) on
[0, 255] with the constants of that convention.
"""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "staging", "flownet2_hip_ssim.h")
U = 2.0 ** -24
C1, C2 = 0.01 ** 2, 0.03 ** 2
FAMILIES = ("noise", "smooth", "identical", "bytes")


def header_macros():
    """{name: value} of the header's numeric ``#define FN2I_*`` lines."""
    out = {}
    for name, val in re.findall(r"^#define (FN2I_[A-Z0-9_]+) ([^\n\\]+)$", open(HEADER).read(), flags=re.M):
        val = val.strip()
        if re.fullmatch(r"[-0-9. +*/()]+", val):
            out[name] = eval(val)   # digits and arithmetic only
    return out


M = header_macros()
TILE_H, TILE_W = M["FN2I_TILE_H"], M["FN2I_TILE_W"]


def constants(family):
    return (C1 * 255.0 ** 2, C2 * 255.0 ** 2) if family == "bytes" else (C1, C2)


def admits(shape, md, border):
    return border == "zero" or (shape[2] > md and shape[3] > md)


def inputs(shape, family, seed=0):
    """(im1, im2, grad_out) as float64 tensors whose values are float32 numbers."""
    N, C, H, W = shape
    rng = np.random.default_rng([seed, FAMILIES.index(family), N, C, H, W])
    if family == "smooth":
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        ph = rng.uniform(0, 2 * np.pi, (N, C, 1, 1))

        def scene(d):
            return 0.5 + 0.3 * np.sin(2 * np.pi * ((xs + d) / 37.0 + ys / 53.0) + ph)

        x, y = scene(0.0), 0.9 * scene(0.5) + 0.02
    else:
        x = rng.uniform(0, 1, shape)
        y = x.copy() if family == "identical" else np.clip(0.7 * x + 0.3 * rng.uniform(0, 1, shape), 0, 1)
        if family == "bytes":
            x, y = 255.0 * x, 255.0 * y
    go = rng.standard_normal(shape)
    return tuple(torch.from_numpy(a.astype(np.float32).astype(np.float64)) for a in (x, y, go))


# ------------------------------------------------------------------ the composition
def compose(x, y, md=1, c1=C1, c2=C2, border="zero"):
    """clamp((1 - SSIM) / 2, 0, 1), N x C x H x W, in the dtype of x: the raw-moment composition of ARFlow and monodepth2."""
    N, C, H, W = x.shape
    k = 2 * md + 1
    if border == "reflect":
        x, y = F.pad(x, (md,) * 4, mode="reflect"), F.pad(y, (md,) * 4, mode="reflect")
    elif H < k or W < k:
        return (x + y) * 0   # no window fits: all zero, and it sends no gradient
    mx, my = F.avg_pool2d(x, k, 1), F.avg_pool2d(y, k, 1)
    sx = F.avg_pool2d(x * x, k, 1) - mx * mx
    sy = F.avg_pool2d(y * y, k, 1) - my * my
    sxy = F.avg_pool2d(x * y, k, 1) - mx * my
    S = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sx + sy + c2))
    dist = torch.clamp((1 - S) / 2, 0, 1)
    return dist if border == "reflect" else F.pad(dist, (md,) * 4)


def valid_mask(shape, md, border, dtype=torch.float64, device="cpu"):
    """N x 1 x H x W: 1 on the inner rectangle (everywhere under reflect)."""
    N, C, H, W = shape
    v = torch.zeros((N, 1, H, W), dtype=dtype, device=device)
    m = 0 if border == "reflect" else md
    v[:, :, m:H - m, m:W - m] = 1.0
    return v


def compose_loss(im1, im2, mask=None, md=1, border="zero", c1=C1, c2=C2):
    """SSIMLoss on the composition: sum(dist valid) / (C sum(valid) + 1e-6)."""
    dist = compose(im1, im2, md, c1, c2, border)
    valid = valid_mask(dist.shape, md, border, dist.dtype, dist.device)
    if mask is not None:
        valid = valid * mask
    return (dist * valid).sum() / (dist.shape[1] * valid.sum() + 1e-6)


# ------------------------------------------------------------------ float64, the header's form, and its bounds
def _windows(t, k):
    """N x C x H' x W' x n: the k x k windows of t, row-major."""
    w = t.unfold(2, k, 1).unfold(3, k, 1)
    return w.reshape(w.shape[:4] + (k * k,))


def _fold(G, shape, md):
    """The adjoint of ReflectionPad2d(md): the padded-domain gradient summed onto the pixels its positions read."""
    z = torch.zeros(shape, dtype=G.dtype, requires_grad=True)
    return torch.autograd.grad(F.pad(z, (md,) * 4, mode="reflect"), z, G)[0]


def reference(x, y, go=None, md=1, c1=C1, c2=C2, border="zero"):
    """dict(out, bound) and, with ``go``, (g1, g2, bound1, bound2, margin): float64 tensors N x C x H x W.  ``margin`` is the least
    distance of an unclamped (1 - S) / 2 from the clamp's ends 0 and 1, in units of the forward bound there (inf without windows)."""
    x, y = x.double(), y.double()
    shape = x.shape
    N, C, H, W = shape
    k = 2 * md + 1
    n = k * k
    zeros = torch.zeros(shape, dtype=torch.float64)
    res = dict(out=zeros, bound=zeros, g1=zeros, g2=zeros, bound1=zeros, bound2=zeros, margin=float("inf"))
    if border == "reflect":
        xp, yp = F.pad(x, (md,) * 4, mode="reflect"), F.pad(y, (md,) * 4, mode="reflect")
    elif H < k or W < k:
        return res
    else:
        xp, yp = x, y
    N1, N4 = n + M["FN2I_BOUND_MEAN"], n + M["FN2I_BOUND_MOMENT"]
    slack, TAP = M["FN2I_BOUND_SLACK"], M["FN2I_BOUND_TAP"]
    wx, wy = _windows(xp, k), _windows(yp, k)
    mx, my = wx.mean(-1), wy.mean(-1)
    ex, ey = wx - mx[..., None], wy - my[..., None]
    sx, sy, sxy = (ex * ex).mean(-1), (ey * ey).mean(-1), (ex * ey).mean(-1)
    X, Y = wx.abs().mean(-1), wy.abs().mean(-1)
    A1, A2, B1, B2 = 2 * mx * my + c1, 2 * sxy + c2, mx * mx + my * my + c1, sx + sy + c2
    S = A1 * A2 / (B1 * B2)
    d = (1 - S) / 2
    # the forward bound
    dmx, dmy = N1 * U * X, N1 * U * Y
    esx, esy = N4 * U * sx + 2 * dmx ** 2, N4 * U * sy + 2 * dmy ** 2
    esxy = N4 * U * torch.sqrt((sx + dmx ** 2) * (sy + dmy ** 2)) + 2 * dmx * dmy
    eA1 = 2 * (my.abs() * dmx + mx.abs() * dmy + dmx * dmy) + 2 * U * (2 * (mx * my).abs() + c1)
    eB1 = 2 * (mx.abs() * dmx + my.abs() * dmy) + dmx ** 2 + dmy ** 2 + 3 * U * B1
    eA2 = 2 * esxy + 2 * U * (2 * sxy.abs() + c2)
    eB2 = esx + esy + 2 * U * B2
    eS = (A2.abs() * eA1 + A1.abs() * eA2) / (B1 * B2) + S.abs() * (eB1 / B1 + eB2 / B2 + 3 * U)
    bound = slack * (eS + U * (1 - S).abs()) / 2
    embed = (lambda t: t) if border == "reflect" else (lambda t: F.pad(t, (md,) * 4))
    res["out"], res["bound"] = embed(d.clamp(0, 1)), embed(bound)
    res["margin"] = float(torch.minimum(d.abs() / bound, (1 - d).abs() / bound).min())
    if go is None:
        return res
    # the gradient: per window the derivatives of S, per tap the header's expression
    gov = go.double() if border == "reflect" else go.double()[:, :, md:H - md, md:W - md]
    gp = torch.where((d >= 0) & (d <= 1), -0.5 * gov, torch.zeros_like(gov))
    E = 1 / (B1 * B2)
    Dsxy, Ds = 2 * A1 * E, -S / B2
    Dmx, Dmy = 2 * my * A2 * E - 2 * mx * S / B1, 2 * mx * A2 * E - 2 * my * S / B1
    eErel = eB1 / B1 + eB2 / B2 + 2 * U
    eDsxy = 2 * E * eA1 + Dsxy.abs() * (eErel + 2 * U)
    eDs = eS / B2 + Ds.abs() * (eB2 / B2 + U)

    def eDm(m_, mo, dm_, dmo, Dm):   # of Dmx: m_ = mx, mo = my
        return (2 * E * (A2.abs() * dmo + mo.abs() * eA2) + (2 * mo * A2 * E).abs() * (eErel + 3 * U) + 2 * (S.abs() * dm_ + m_.abs() * eS) / B1
                + (2 * m_ * S / B1).abs() * (eB1 / B1 + 3 * U) + U * Dm.abs())

    eDmx, eDmy = eDm(mx, my, dmx, dmy, Dmx), eDm(my, mx, dmy, dmx, Dmy)
    g = gp.abs() / n
    Hv, Wv = mx.shape[2:]
    G1, G2, Bd1, Bd2 = (torch.zeros_like(xp) for _ in range(4))
    for dy in range(k):
        for dx in range(k):
            sl = (slice(None), slice(None), slice(dy, dy + Hv), slice(dx, dx + Wv))
            qx, qy = xp[sl] - mx, yp[sl] - my
            t1 = Dmx + 2 * Ds * qx + Dsxy * qy
            t2 = Dmy + 2 * Ds * qy + Dsxy * qx
            G1[sl] += gp / n * t1
            G2[sl] += gp / n * t2
            ax, ay = qx.abs(), qy.abs()
            Bd1[sl] += (g * (eDmx + 2 * eDs * ax + eDsxy * ay + 2 * Ds.abs() * (dmx + U * ax) + Dsxy.abs() * (dmy + U * ay))
                        + TAP * U * g * (Dmx.abs() + 2 * Ds.abs() * ax + Dsxy.abs() * ay) + N1 * U * g * t1.abs())
            Bd2[sl] += (g * (eDmy + 2 * eDs * ay + eDsxy * ax + 2 * Ds.abs() * (dmy + U * ay) + Dsxy.abs() * (dmx + U * ax))
                        + TAP * U * g * (Dmy.abs() + 2 * Ds.abs() * ay + Dsxy.abs() * ax) + N1 * U * g * t2.abs())
    if border == "reflect":
        G1, G2, Bd1, Bd2 = (_fold(t, shape, md) for t in (G1, G2, Bd1, Bd2))
    res.update(g1=G1, g2=G2, bound1=slack * Bd1, bound2=slack * Bd2)
    return res
