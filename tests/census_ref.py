"""float64 reference of the ternary census distance (include/flownet2_hip_census.h), written from the header's formulas with numpy
shifts -- not from the kernels' tiling; ``compose``, the PyTorch composition (identity-filter ``conv2d`` unfold, soft sign, robust
distance, mean or sum, border mask); ``emulate``, the header's operation list in numpy float32; and the image families the tests
share.  Test infrastructure only.

The grey intensities are restated in numpy float32 in the header's operation order, so that everything after them starts from the
numbers the kernels start from; everything after them is float64.

    g = ((r 0.2989f + g 0.5870f) + b 0.1140f) scale      x_i = g_i[p + k] - g_i[p]      f(x) = x / sqrt(0.81 + x^2)
    out[p] = w sum_k h(f(x_1) - f(x_2))                  h(d) = d^2 / (0.1 + d^2)        0 on the border ring of width md
"""
import os
import re

import numpy as np

CW = (np.float32(0.2989), np.float32(0.5870), np.float32(0.1140))

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flownet2_hip_census.h")


def header_macros():
    """The integer macros of the header: FN2C_ABI_VERSION, FN2C_TILE_H, FN2C_TILE_W, FN2C_PAD, FN2C_MAX_DISTANCE and the two
    bound exponents FN2C_FWD_BOUND_LOG2, FN2C_BWD_BOUND_LOG2."""
    txt = open(_HDR).read()
    return {k: int(v) for k, v in re.findall(r"^#define (FN2C_[A-Z0-9_]+) (-?\d+)\s*$", txt, flags=re.M)}


def lds_bytes(planes, md):
    """FN2C_LDS_BYTES(planes, md), evaluated from the header's macros."""
    m = header_macros()
    return planes * 4 * (m["FN2C_TILE_H"] + 2 * md) * (m["FN2C_TILE_W"] + 2 * md + m["FN2C_PAD"])


def weight(md, normalize):
    K = (2 * md + 1) ** 2
    return 1.0 / K if normalize else 1.0


def grey(im, scale):
    """N x H x W float32: the grey intensity in the header's fp32 operation order."""
    im = np.asarray(im, dtype=np.float32)
    s = np.float32(scale)
    if im.shape[1] == 1:
        return (im[:, 0] * s).astype(np.float32)
    assert im.shape[1] == 3
    g = ((im[:, 0] * CW[0]).astype(np.float32) + (im[:, 1] * CW[1]).astype(np.float32)).astype(np.float32)
    g = (g + (im[:, 2] * CW[2]).astype(np.float32)).astype(np.float32)
    return (g * s).astype(np.float32)


def f(x):
    return x / np.sqrt(0.81 + x * x)


def df(x):
    return 0.81 / (0.81 + x * x) ** 1.5


def h(d):
    return d * d / (0.1 + d * d)


def dh(d):
    return 0.2 * d / (0.1 + d * d) ** 2


def offsets(md):
    return [(dy, dx) for dy in range(-md, md + 1) for dx in range(-md, md + 1) if (dy, dx) != (0, 0)]


def _shift(a, dy, dx):
    """b[..., y, x] = a[..., y + dy, x + dx], 0 outside the image."""
    H, W = a.shape[-2:]
    b = np.zeros_like(a)
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[..., yd, xd] = a[..., ys, xs]
    return b


def inner(H, W, md):
    """H x W bool: True inside the border ring of width md (all False if H or W < 2 md + 1)."""
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy >= md) & (yy < H - md) & (xx >= md) & (xx < W - md)


def forward_grey(g1, g2, md, normalize=True):
    """N x 1 x H x W float64 from the grey planes (N x H x W)."""
    g1, g2 = np.asarray(g1, np.float64), np.asarray(g2, np.float64)
    acc = np.zeros_like(g1)
    for dy, dx in offsets(md):
        acc += h(f(_shift(g1, dy, dx) - g1) - f(_shift(g2, dy, dx) - g2))
    return (weight(md, normalize) * acc * inner(*g1.shape[-2:], md))[:, None]


def forward(im1, im2, md=3, scale=255.0, normalize=True):
    return forward_grey(grey(im1, scale), grey(im2, scale), md, normalize)


def forward_bound(md, normalize=True):
    """|err| <= 2^FN2C_FWD_BOUND_LOG2 w K, the same for every pixel."""
    return 2.0 ** header_macros()["FN2C_FWD_BOUND_LOG2"] * weight(md, normalize) * (2 * md + 1) ** 2


def backward_grey(g1, g2, go, md, normalize=True):
    """The header's gather form: (grad_g1, grad_g2, A_g), each N x H x W float64; A_g = w sum_{k != 0} (|gO'[q]| + |gO'[q - k]|)."""
    g1, g2 = np.asarray(g1, np.float64), np.asarray(g2, np.float64)
    gop = np.asarray(go, np.float64)[:, 0] * inner(*g1.shape[-2:], md)
    w = weight(md, normalize)
    a1, a2, A = np.zeros_like(g1), np.zeros_like(g1), np.zeros_like(g1)
    for dy, dx in offsets(md):
        x1, x2 = g1 - _shift(g1, -dy, -dx), g2 - _shift(g2, -dy, -dx)       # q - k
        gk = _shift(gop, -dy, -dx)
        t = (gop + gk) * dh(f(x1) - f(x2))
        a1 += t * df(x1)
        a2 -= t * df(x2)
        A += np.abs(gop) + np.abs(gk)
    return w * a1, w * a2, w * A


def backward(im1, im2, go, md=3, scale=255.0, normalize=True):
    """(grad_im1, grad_im2, A): N x C x H x W float64 each; the gradient bound is 2^FN2C_BWD_BOUND_LOG2 A."""
    C = np.asarray(im1).shape[1]
    a1, a2, A = backward_grey(grey(im1, scale), grey(im2, scale), go, md, normalize)
    cw = np.array([float(c) for c in CW] if C == 3 else [1.0])[None, :, None, None] * float(np.float32(scale))
    return cw * a1[:, None], cw * a2[:, None], np.abs(cw) * A[:, None]


def backward_bound(A):
    return 2.0 ** header_macros()["FN2C_BWD_BOUND_LOG2"] * A


# ------------------------------------------------------------------ the PyTorch composition
def compose_grey(g1, g2, md, normalize=True):
    """What a user writes without the layer, from grey planes N x 1 x H x W of any float dtype: the identity-filter conv2d unfold
    (zero padding), t / sqrt(0.81 + t^2), d^2 / (0.1 + d^2), mean or sum over the K channels, the border mask."""
    import torch
    import torch.nn.functional as F
    P = 2 * md + 1
    K = P * P
    filt = torch.eye(K, dtype=g1.dtype, device=g1.device).view(K, 1, P, P)

    def transform(g):
        t = F.conv2d(g, filt, padding=md) - g
        return t / torch.sqrt(0.81 + t * t)

    d = (transform(g1) - transform(g2)) ** 2
    dist = d / (0.1 + d)
    dist = dist.mean(1, keepdim=True) if normalize else dist.sum(1, keepdim=True)
    mask = torch.zeros_like(dist)
    H, W = dist.shape[2:]
    if H > 2 * md and W > 2 * md:
        mask[:, :, md:H - md, md:W - md] = 1
    return dist * mask


def torch_grey(im, scale):
    """The grey plane N x 1 x H x W in the tensor's own dtype, the header's operation order."""
    if im.shape[1] == 1:
        return im * scale
    return (((im[:, 0] * float(CW[0]) + im[:, 1] * float(CW[1])) + im[:, 2] * float(CW[2])) * scale).unsqueeze(1)


def compose(im1, im2, md=3, scale=255.0, normalize=True):
    return compose_grey(torch_grey(im1, scale), torch_grey(im2, scale), md, normalize)


def compose_loss(g1, g2, mask=None, md=3, q=0.4, eps=0.01):
    """CensusLoss as a composition from grey planes N x 1 x H x W: sum((dist + eps)^q valid) / (sum(valid) + 1e-6)."""
    import torch
    dist = compose_grey(g1, g2, md, True)
    valid = torch.zeros_like(dist)
    H, W = dist.shape[2:]
    valid[:, :, md:H - md, md:W - md] = 1
    if mask is not None:
        valid = valid * mask
    return ((dist + eps) ** q * valid).sum() / (valid.sum() + 1e-6)


# ------------------------------------------------------------------ inputs
def image_pair(shape, seed):
    """im1 uniform in [0, 1), im2 = im1 + 5 % noise clipped to [0, 1] (a warped second frame), grad_out standard normal."""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    im1 = rng.random(shape).astype(np.float32)
    im2 = np.clip(im1 + 0.05 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)
    go = rng.standard_normal((N, 1, H, W)).astype(np.float32)
    return im1, im2, go


FAMILIES = ("noise", "knee", "opposed", "flat", "graded", "seams")
GRADED_EXPONENTS = (-130, -40, -12, 0, 12, 40, 59)
GRADED_BAND = 10
# (family, scale) as the tests run them: every family at its own scale, ``noise`` and ``seams`` at further ones
FAMILY_SCALES = (("noise", 255.0), ("noise", -255.0), ("noise", 1.0), ("noise", 2.0 ** -30), ("knee", 255.0), ("opposed", 255.0),
                 ("flat", 255.0), ("graded", 1.0), ("seams", 255.0), ("seams", 1.0))


def grad_out(shape, seed):
    """N x 1 x H x W float32, standard normal."""
    return np.random.default_rng(seed).standard_normal((shape[0], 1) + tuple(shape[2:])).astype(np.float32)


def _taps(g, md):
    """K - 1 x N x h x w float64: x = g[p + k] - g[p] of every interior pixel p and offset k."""
    g = np.asarray(g, np.float64)
    H, W = g.shape[-2:]
    return np.stack([g[:, md + dy:H - md + dy, md + dx:W - md + dx] - g[:, md:H - md, md:W - md] for dy, dx in offsets(md)])


def image_family(name, shape, seed):
    """(im1, im2, scale): float32 N x C x H x W each, and the scale the family is meant for.  Each family asserts on its own
    output what it is for (on planes of at least 17 x 67, max_distance 3), so that a change of constants cannot turn it benign:
      noise    ``image_pair``: im1 uniform in [0, 1), im2 = im1 + 5 % noise; scale 255
      knee     a contrast of 2 / 255 around 0.5, im2 = im1 + noise of a quarter of that: the grey differences stay where f' > 0.1
      opposed  im2 = 1 - im1: f_1 and f_2 have opposite signs, |d| near 2
      flat     im1 constant 0.25, im2 = im1 + 2^-21 N(0, 1): an output below 10^-5
      graded   scale 1; column bands of GRADED_BAND columns carry magnitudes 2^e, e cycling through GRADED_EXPONENTS, im1 uniform in
               [1/4, 1) times that, im2 = im1 (1 + 5 % noise): subnormal intensities next to intensities of 2^59
      seams    a +-1 checkerboard of period 1 left of column 64 and, right of it, a single step between rows 15 and 16; im2 is im1
               moved by one column: transitions on the tile seams.  Meant for scale 255 and scale 1."""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    big = H >= 17 and W >= 67
    scale = 255.0
    if name == "noise":
        im1, im2, _ = image_pair(shape, seed)
    elif name == "knee":
        im1 = (0.5 + (2.0 / 255) * (rng.random(shape) - 0.5)).astype(np.float32)
        im2 = (im1 + (0.5 / 255) * rng.standard_normal(shape)).astype(np.float32)
        if big:
            x1 = _taps(grey(im1, scale), 3)
            assert (np.abs(x1) < 1.75).mean() >= 0.5 and df(1.75) > 0.1
    elif name == "opposed":
        im1 = rng.random(shape).astype(np.float32)
        im2 = (np.float32(1) - im1).astype(np.float32)
        if big:
            d = f(_taps(grey(im1, scale), 3)) - f(_taps(grey(im2, scale), 3))
            assert np.median(np.abs(d)) > 1.5
    elif name == "flat":
        im1 = np.full(shape, 0.25, np.float32)
        im2 = (im1 + 2.0 ** -21 * rng.standard_normal(shape)).astype(np.float32)
        if big:
            out = forward(im1, im2, 3, scale, True)
            assert out.max() > 0 and out.max() < 1e-5
    elif name == "graded":
        scale = 1.0
        band = np.array(GRADED_EXPONENTS, np.float64)[(np.arange(W) // GRADED_BAND) % len(GRADED_EXPONENTS)]
        im1 = ((0.25 + 0.75 * rng.random(shape)) * 2.0 ** band).astype(np.float32)
        im2 = (im1.astype(np.float64) * (1 + 0.05 * rng.standard_normal(shape))).astype(np.float32)
        if big:
            for im in (im1, im2):
                g = np.abs(grey(im, scale).astype(np.float64))
                assert 2.0 ** 57 <= g.max() < 2.0 ** 60, g.max()
            tiny = (np.abs(im1) < 2.0 ** -126) & (im1 != 0)
            assert tiny.mean() >= 0.05
    elif name == "seams":
        yy, xx = np.mgrid[0:H, 0:W]
        plane = np.where(xx < 64, 1.0 - 2.0 * ((xx + yy) % 2), np.where(yy < 16, 1.0, -1.0)).astype(np.float32)
        im1 = np.broadcast_to(plane, shape).copy()
        im2 = np.roll(im1, 1, axis=3)
        if big:
            assert (im1[..., 15, 64:] != im1[..., 16, 64:]).all() and (im1[..., 15, :64] != im1[..., 16, :64]).all()
            assert (im1[..., :, 63] != im1[..., :, 64]).any() and (im1[..., :, 62] != im1[..., :, 63]).all()
    else:
        raise ValueError(f"no image family {name!r}")
    assert im1.dtype == im2.dtype == np.float32 and np.isfinite(im1).all() and np.isfinite(im2).all()
    return im1, im2, scale


# ------------------------------------------------------------------ the header's operation list in float32
def emulate(im1, im2, go, md=3, scale=255.0, normalize=True, mutate=None):
    """(out, grad_im1, grad_im2) in float32, following include/flownet2_hip_census.h operation by operation in numpy float32
    (every operation rounded on its own, rsq and rcp correctly rounded), in the header's summation order.  ``mutate`` plants
    one mistake, for the tests that show which family catches it:
      "clamped_grey"  the grey intensity clamped to [0, 255], as if every image were in [0, 1] and every scale 255
      "abs_scale"     the gradient scaled by |scale| instead of scale"""
    f32 = np.float32
    im1, im2 = np.asarray(im1, f32), np.asarray(im2, f32)
    N, C, H, W = im1.shape
    s = f32(scale)

    def grey_of(im):
        return np.clip(grey(im, scale), f32(0), f32(255)) if mutate == "clamped_grey" else grey(im, scale)

    def rsq(v):
        return (1.0 / np.sqrt(v.astype(np.float64))).astype(f32)

    def rcp(v):
        return (1.0 / v.astype(np.float64)).astype(f32)

    g1, g2 = grey_of(im1), grey_of(im2)
    w = f32(1.0 / (2 * md + 1) ** 2) if normalize else f32(1)
    ins = inner(H, W, md)
    gop = np.where(ins, np.asarray(go, f32)[:, 0], f32(0))
    total, a1, a2 = np.zeros((N, H, W), f32), np.zeros((N, H, W), f32), np.zeros((N, H, W), f32)
    with np.errstate(under="ignore"):
        for dx in range(-md, md + 1):
            col, c1, c2 = np.zeros((N, H, W), f32), np.zeros((N, H, W), f32), np.zeros((N, H, W), f32)
            for dy in range(-md, md + 1):
                if (dy, dx) == (0, 0):
                    continue
                # forward: x = g[p + k] - g[p]
                x1, x2 = _shift(g1, dy, dx) - g1, _shift(g2, dy, dx) - g2
                d = x1 * rsq(f32(0.81) + x1 * x1) - x2 * rsq(f32(0.81) + x2 * x2)
                d2 = d * d
                col = col + d2 * rcp(f32(0.1) + d2)
                # backward: x = g[q] - g[q + k]
                x1, x2 = g1 - _shift(g1, dy, dx), g2 - _shift(g2, dy, dx)
                r1, r2 = rsq(f32(0.81) + x1 * x1), rsq(f32(0.81) + x2 * x2)
                d = x1 * r1 - x2 * r2
                q = rcp(f32(0.1) + d * d)
                t = (gop + _shift(gop, dy, dx)) * ((f32(0.2) * d) * (q * q))
                c1 = c1 + t * (f32(0.81) * ((r1 * r1) * r1))
                c2 = c2 - t * (f32(0.81) * ((r2 * r2) * r2))
            total, a1, a2 = total + col, a1 + c1, a2 + c2
        out = np.where(ins, w * total, f32(0))[:, None]
        sg = np.abs(s) if mutate == "abs_scale" else s
        cw = np.array(CW if C == 3 else [f32(1)], f32)[None, :, None, None] * sg if C == 3 else np.full((1, 1, 1, 1), sg, f32)
        return out.astype(f32), (cw * (w * a1)[:, None]).astype(f32), (cw * (w * a2)[:, None]).astype(f32)
