"""float64 reference of the edge-aware smoothness term (include/flownet2_hip_smooth.h), written from the header's formulas with
numpy slices -- not from the kernels' tiling: the forward, the backward (a scatter here, a gather in the kernels), S, both bound
arrays; ``compose``, the PyTorch composition a user writes without the layer (slices, differentiated by autograd); and the input
families the tests share.  Test infrastructure only.

Everything is evaluated in float64 on the fp32 inputs; alpha and eps are the fp32 numbers the C ABI receives.

    dI_c = I_c[p + k] - I_c[p]      e = mean_c |alpha dI_c| or mean_c (alpha dI_c)^2      w = exp(-e)
    d_f = first or second difference of the flow      rho = sqrt(d^2 + eps^2)      out = w sum_f rho      0 where the stencil does not fit
"""
import os
import re

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -126
EDGES = ("exponential", "gaussian")
# (alpha, amplitude) of the image family: e stays at or below about 56, so w stays a normal number
IMAGE_FAMILIES = ((150.0, 0.05), (10.0, 0.75))

_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flownet2_hip_smooth.h")


def header_macros():
    """The integer macros of the header: FN2M_ABI_VERSION, FN2M_TILE_H, FN2M_TILE_W, FN2M_HALO_X, FN2M_MAX_ORDER,
    FN2M_MAX_FLOW_CHANNELS, the two edge codes and the bound constants FN2M_BOUND_A, FN2M_BOUND_E."""
    txt = open(_HDR).read()
    return {k: int(v) for k, v in re.findall(r"^#define (FN2M_[A-Z0-9_]+) (-?\d+)\s*$", txt, flags=re.M)}


def lds_bytes(planes, k, bwd):
    """FN2M_LDS_BYTES(planes, k, bwd), evaluated from the header's macros."""
    m = header_macros()
    return planes * 4 * (m["FN2M_TILE_H"] + (2 * k if bwd else k)) * (m["FN2M_TILE_W"] + (2 if bwd else 1) * m["FN2M_HALO_X"])


def _sl(axis, start, stop):
    s = [slice(None)] * 4
    s[axis] = slice(start, stop)
    return tuple(s)


def _direction(flow, image, axis, k, edge, alpha, eps):
    """The quantities of one direction (axis 3: x, axis 2: y) on its valid cells, or None if the stencil fits nowhere:
    e, w (N x 1 x h x w), d, S, rho, drho (rho'), ddrho (rho'' = eps^2 / rho^3), each N x F x h x w."""
    f, im = np.asarray(flow, np.float64), np.asarray(image, np.float64)
    L = f.shape[axis]
    if L <= k:
        return None
    alpha, eps = float(np.float32(alpha)), float(np.float32(eps))
    t = alpha * (im[_sl(axis, k, L)] - im[_sl(axis, 0, L - k)])
    e = (np.abs(t) if edge == "exponential" else t * t).mean(axis=1, keepdims=True)
    if k == 1:
        d = f[_sl(axis, 1, L)] - f[_sl(axis, 0, L - 1)]
        S = np.zeros_like(d)
    else:
        a, b = f[_sl(axis, 2, L)] - f[_sl(axis, 1, L - 1)], f[_sl(axis, 1, L - 1)] - f[_sl(axis, 0, L - 2)]
        d, S = a - b, np.abs(a) + np.abs(b)
    rho = np.sqrt(d * d + eps * eps)
    safe = np.where(rho > 0, rho, 1.0)
    drho = np.where(rho > 0, d / safe, 0.0)
    ddrho = np.where(rho > 0, eps * eps / safe ** 3, 0.0)
    return dict(e=e, w=np.exp(-e), d=d, S=S, rho=rho, drho=drho, ddrho=ddrho)


def _rel(q):
    m = header_macros()
    return m["FN2M_BOUND_A"] + m["FN2M_BOUND_E"] * q["e"]


def forward(flow, image, order=1, edge="exponential", alpha=150.0, eps=0.001):
    """(out, bound): N x 2 x H x W float64 each; bound is the header's forward bound, 0 where the stencil does not fit."""
    N, F, H, W = np.asarray(flow).shape
    out, bound = np.zeros((N, 2, H, W)), np.zeros((N, 2, H, W))
    for plane, axis in ((0, 3), (1, 2)):
        q = _direction(flow, image, axis, order, edge, alpha, eps)
        if q is None:
            continue
        L = (H, W)[axis - 2]
        dst = (slice(None), slice(plane, plane + 1)) + _sl(axis, 0, L - order)[2:]
        out[dst] = q["w"] * q["rho"].sum(axis=1, keepdims=True)
        bound[dst] = (U * (_rel(q) * q["w"] * q["rho"] + 2 * q["w"] * q["S"]) + FLOOR * q["rho"]).sum(axis=1, keepdims=True)
    return out, bound


def backward(flow, image, go, order=1, edge="exponential", alpha=150.0, eps=0.001):
    """(grad_flow, bound): N x F x H x W float64 each.  grad_out counts only where the stencil fits (a select: NaN elsewhere is
    ignored); bound = u sum over the taps of |coef| T."""
    N, F, H, W = np.asarray(flow).shape
    grad, bound = np.zeros((N, F, H, W)), np.zeros((N, F, H, W))
    go = np.asarray(go, np.float64)
    coefs = (-1.0, 1.0) if order == 1 else (1.0, -2.0, 1.0)
    for plane, axis in ((0, 3), (1, 2)):
        q = _direction(flow, image, axis, order, edge, alpha, eps)
        if q is None:
            continue
        L = (H, W)[axis - 2]
        g = go[(slice(None), slice(plane, plane + 1)) + _sl(axis, 0, L - order)[2:]]
        t = g * q["w"] * q["drho"]
        T = np.abs(g) * (q["w"] * (_rel(q) * np.abs(q["drho"]) + 2 * q["S"] * q["ddrho"]) + FLOOR / U)
        for j, c in enumerate(coefs):
            dst = _sl(axis, j, L - order + j)
            grad[dst] += c * t
            bound[dst] += abs(c) * U * T
    return grad, bound


# ------------------------------------------------------------------ the PyTorch composition
def compose(flow, image, order=1, edge="exponential", alpha=150.0, eps=0.001):
    """What a user writes without the layer, in the tensors' own dtype: image gradients with stride k, abs or square, the channel
    mean, exp, flow gradients taken once or twice, the robust function, the product, and zero padding to N x 2 x H x W."""
    import torch
    import torch.nn.functional as Fn
    k = order
    alpha, eps = float(np.float32(alpha)), float(np.float32(eps))

    def weight(dI):
        a = alpha * dI
        return torch.exp(-(a.abs() if edge == "exponential" else a * a).mean(1, keepdim=True))

    def rho(d):
        return torch.sqrt(d * d + eps * eps) if eps > 0 else d.abs()

    N, F, H, W = flow.shape
    px, py = flow.new_zeros(N, 1, H, 0), flow.new_zeros(N, 1, 0, W)
    if W > k:
        fx = flow
        for _ in range(k):
            fx = fx[:, :, :, 1:] - fx[:, :, :, :-1]
        px = weight(image[:, :, :, k:] - image[:, :, :, :-k]) * rho(fx).sum(1, keepdim=True)
    if H > k:
        fy = flow
        for _ in range(k):
            fy = fy[:, :, 1:] - fy[:, :, :-1]
        py = weight(image[:, :, k:] - image[:, :, :-k]) * rho(fy).sum(1, keepdim=True)
    return torch.cat([Fn.pad(px, (0, W - px.shape[3], 0, 0)), Fn.pad(py, (0, 0, 0, H - py.shape[2]))], 1)


def loss_of(out, F, order):
    """UFlow's reduction of the two planes (numpy or torch): the mean over every flow-gradient element per direction, halved."""
    N, _, H, W = out.shape
    nx, ny = N * F * H * (W - order), N * F * (H - order) * W
    lx = out[:, 0].sum() / nx if nx > 0 else 0.0
    ly = out[:, 1].sum() / ny if ny > 0 else 0.0
    return (lx + ly) / 2


def compose_loss(flow, image, order=1, edge="exponential", alpha=150.0, eps=0.001):
    """UFlow's two means, written as UFlow writes them: mean over the valid slices of each direction."""
    k = order
    out = compose(flow, image, order, edge, alpha, eps)
    H, W = out.shape[2:]
    F = flow.shape[1]
    lx = out[:, 0, :, :W - k].mean() / F if W > k else 0.0
    ly = out[:, 1, :H - k, :].mean() / F if H > k else 0.0
    return (lx + ly) / 2


# ------------------------------------------------------------------ inputs
def _box9(a):
    """9 x 9 box mean with edge padding."""
    p = np.pad(a, ((0, 0), (0, 0), (4, 4), (4, 4)), mode="edge")
    H, W = a.shape[2:]
    acc = np.zeros_like(a)
    for dy in range(9):
        for dx in range(9):
            acc += p[:, :, dy:dy + H, dx:dx + W]
    return acc / 81.0


def inputs(shape, family, seed):
    """(flow, image, grad_out, alpha) for shape = (N, F, C, H, W): the image 0.5 + amp (uniform - 0.5) with IMAGE_FAMILIES[family]'s
    (alpha, amp), the flow a 9 x 9 box-smoothed N(0, 20^2) field plus 0.3 N(0, 1), grad_out standard normal."""
    N, F, C, H, W = shape
    alpha, amp = IMAGE_FAMILIES[family]
    rng = np.random.default_rng(seed)
    image = (0.5 + amp * (rng.random((N, C, H, W)) - 0.5)).astype(np.float32)
    flow = (_box9(20.0 * rng.standard_normal((N, F, H, W))) + 0.3 * rng.standard_normal((N, F, H, W))).astype(np.float32)
    go = rng.standard_normal((N, 2, H, W)).astype(np.float32)
    return flow, image, go, alpha


def dyadic_flow(shape, seed, patch=3):
    """N x F x H x W float32 of multiples of 1/8 with |f| <= 64, constant on patch x patch squares: every first and second
    difference is exact in fp32, and many are 0."""
    N, F, C, H, W = shape
    rng = np.random.default_rng(seed)
    coarse = rng.integers(-512, 513, (N, F, -(-H // patch), -(-W // patch))).astype(np.float32) / np.float32(8)
    return np.repeat(np.repeat(coarse, patch, axis=2), patch, axis=3)[:, :, :H, :W].copy()
