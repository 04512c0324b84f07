"""float64 reference of the edge-aware smoothness term (include/flownet2_hip_smooth.h), written from the header's formulas with
numpy slices -- not from the kernels' tiling: the forward, the backward (a scatter here, a gather in the kernels), S, both bound
arrays (and the first-order gradient bound the header stated at first); ``compose``, the PyTorch composition a user writes without
the layer (slices, differentiated by autograd); ``emulate``, the header's operation list in numpy float32; and the input families the
tests share.  Test infrastructure only.

Everything is evaluated in float64 on the fp32 inputs; alpha and eps are the fp32 numbers the C ABI receives.

    dI_c = I_c[p + k] - I_c[p]      e = mean_c |alpha dI_c| or mean_c (alpha dI_c)^2      w = exp(-e)
    d_f = first or second difference of the flow      rho = sqrt(d^2 + eps^2)      out = w sum_f rho      0 where the stencil does not fit
"""
import os
import re

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -126
TINY = 2.0 ** -149
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
    # the corrected gradient bound's d term: dd bounds |d^ - d|, D the change of rho' it can cause
    dd = U * np.abs(d) if k == 1 else U * ((1 + U) * S + np.abs(d))
    if eps > 0:
        lo = np.maximum(np.abs(d) - dd, 0.0)
        D = np.minimum(2.0, dd * (eps * eps / (lo * lo + eps * eps) ** 1.5))
    else:
        D = np.where((np.abs(d) <= dd) & (dd > 0), 2.0, 0.0)
    return dict(e=e, w=np.exp(-e), d=d, S=S, rho=rho, drho=drho, ddrho=ddrho, dd=dd, D=D)


def _rel(q):
    """(FN2M_BOUND_A + FN2M_BOUND_E e) w, the relative part of both bounds; 0 where float64's exp(-e) is 0."""
    m = header_macros()
    return np.where(q["w"] > 0, (m["FN2M_BOUND_A"] + m["FN2M_BOUND_E"] * q["e"]) * q["w"], 0.0)


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
        bound[dst] = (U * (_rel(q) * q["rho"] + 2 * q["w"] * q["S"]) + FLOOR * q["rho"]).sum(axis=1, keepdims=True)
        bound[dst] += np.where((out[dst] > 0) & (out[dst] < 2 * FLOOR), TINY, 0.0)      # the product's rounding once it is subnormal
    return out, bound


def backward(flow, image, go, order=1, edge="exponential", alpha=150.0, eps=0.001, corrected=False):
    """(grad_flow, bound): N x F x H x W float64 each.  grad_out counts only where the stencil fits (a select: NaN elsewhere is
    ignored); bound = u sum over the taps of |coef| T, the header's first-order bound of ABI 1.  With ``corrected`` a third
    array follows: the header's gradient bound as it stands now, whose d term is max(2 u S eps^2 / rho^3, 2 D)."""
    N, F, H, W = np.asarray(flow).shape
    grad, bound, fixed = np.zeros((N, F, H, W)), np.zeros((N, F, H, W)), np.zeros((N, F, H, W))
    go = np.asarray(go, np.float64)
    coefs = (-1.0, 1.0) if order == 1 else (1.0, -2.0, 1.0)
    for plane, axis in ((0, 3), (1, 2)):
        q = _direction(flow, image, axis, order, edge, alpha, eps)
        if q is None:
            continue
        L = (H, W)[axis - 2]
        g = go[(slice(None), slice(plane, plane + 1)) + _sl(axis, 0, L - order)[2:]]
        t = g * q["w"] * q["drho"]
        T = np.abs(g) * (_rel(q) * np.abs(q["drho"]) + q["w"] * (2 * q["S"] * q["ddrho"]) + FLOOR / U)
        Tc = np.abs(g) * (_rel(q) * np.abs(q["drho"]) + q["w"] * np.maximum(2 * q["S"] * q["ddrho"], 2 * q["D"] / U) + FLOOR / U)
        Tc += np.where((t != 0) & (np.abs(t) < 2 * FLOOR), TINY / U, 0.0)      # the two products' rounding once t is subnormal
        for j, c in enumerate(coefs):
            dst = _sl(axis, j, L - order + j)
            grad[dst] += c * t
            bound[dst] += abs(c) * U * T
            fixed[dst] += abs(c) * U * Tc
    return (grad, bound, fixed) if corrected else (grad, bound)


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


NEW_FAMILIES = ("edges", "ramp", "offset", "graded", "alpha0")
GRADED_EXPONENTS = (-70, -30, 0, 30, 59)
GRADED_EPS = (0.0, 2.0 ** -60, 0.001, 16.0)
GRADED_BAND = 26
RAMP_PERIOD = 16


def inputs(shape, family, seed):
    """(flow, image, grad_out, alpha) for shape = (N, F, C, H, W).  Families 0 and 1: the image 0.5 + amp (uniform - 0.5) with
    IMAGE_FAMILIES[family]'s (alpha, amp), the flow a 9 x 9 box-smoothed N(0, 20^2) field plus 0.3 N(0, 1), grad_out standard
    normal.  The named families change one of the three and assert (``check_family``) that they still do what they are for:
      edges    image of 3 x 3 blocks with levels {0, 1, 2, 3} 0.95 / 3 on all channels, alpha 150: e = 0, e in the flush band of
               the weight (87.4 .. 103.3), e > 104 and, gaussian, e > 10^4
      ramp     flow 2^20 x + 2^18 y + 0.05 N(0, 1), restarting every RAMP_PERIOD columns and rows: the second difference cancels
               2^21 against an O(0.1) result, and only next to a restart is the flow fine enough for 0 < |d| <= u S, so the
               restarts keep the share of such cells independent of the plane's size
      offset   flow 2^22 + N(0, 1)
      graded   the flow of family 0 scaled to max |f| in [1/2, 1), then column bands of GRADED_BAND columns scaled by 2^e, e
               cycling through GRADED_EXPONENTS; |f| < 2^59.  To be combined with GRADED_EPS.
      alpha0   alpha = 0 on the high-contrast image of family 1 and ``dyadic_flow``: w = 1, every rho exact with eps = 0"""
    N, F, C, H, W = shape
    alpha, amp = IMAGE_FAMILIES[family if family in (0, 1) else 1 if family == "alpha0" else 0]
    rng = np.random.default_rng(seed)
    image = (0.5 + amp * (rng.random((N, C, H, W)) - 0.5)).astype(np.float32)
    flow = (_box9(20.0 * rng.standard_normal((N, F, H, W))) + 0.3 * rng.standard_normal((N, F, H, W))).astype(np.float32)
    go = rng.standard_normal((N, 2, H, W)).astype(np.float32)
    if family in (0, 1):
        return flow, image, go, alpha
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if family == "edges":
        levels = rng.integers(0, 4, (N, 1, -(-H // 3), -(-W // 3)))
        levels = np.repeat(np.repeat(levels, 3, axis=2), 3, axis=3)[:, :, :H, :W]
        image = np.broadcast_to((levels * (0.95 / 3)).astype(np.float32), (N, C, H, W)).copy()
    elif family == "ramp":
        flow = (2.0 ** 20 * (xx % RAMP_PERIOD) + 2.0 ** 18 * (yy % RAMP_PERIOD) + 0.05 * rng.standard_normal((N, F, H, W))).astype(np.float32)
    elif family == "offset":
        flow = (2.0 ** 22 + rng.standard_normal((N, F, H, W))).astype(np.float32)
    elif family == "graded":
        top = float(np.abs(flow).max())
        flow = flow * np.float32(2.0 ** -(np.floor(np.log2(top)) + 1))
        band = np.array(GRADED_EXPONENTS, np.float64)[(np.arange(W) // GRADED_BAND) % len(GRADED_EXPONENTS)]
        flow = (flow * (2.0 ** band).astype(np.float32)).astype(np.float32)
    elif family == "alpha0":
        flow, alpha = dyadic_flow(shape, seed), 0.0
    else:
        raise ValueError(f"no input family {family!r}")
    check_family(family, flow, image, alpha)
    return flow, image, go, alpha


def check_family(family, flow, image, alpha):
    """The conditions that make a named family what it is; an AssertionError if a change of constants has turned it benign.
    Conditions on a count need the stencil to fit and are asked of planes of at least 17 x 65."""
    N, F, H, W = flow.shape
    big = H >= 17 and W >= 65
    assert np.isfinite(flow).all() and np.isfinite(image).all() and np.abs(flow).max() < 2.0 ** 60
    if family == "edges":
        for k in (1, 2):
            for edge in EDGES:
                q = _direction(flow, image, 3, k, edge, alpha, 0.001)
                e = q["e"]
                if big:
                    assert (e == 0).any() and (e > 104).any(), (k, edge)
                    if edge == "exponential":
                        assert ((e > 87.4) & (e < 103.3)).any(), k
                    else:
                        assert (e > 1e4).any(), k
                go = np.ones((N, 2, H, W), np.float32)
                _, fb = forward(flow, image, k, edge, alpha, 0.001)
                _, gb, gc = backward(flow, image, go, k, edge, alpha, 0.001, corrected=True)
                assert np.isfinite(fb).all() and np.isfinite(gb).all() and np.isfinite(gc).all()
    elif family == "ramp":
        near = []
        for axis in (2, 3):
            q = _direction(flow, image, axis, 2, "exponential", alpha, 0.0)
            near.append(((np.abs(q["d"]) > 0) & (np.abs(q["d"]) <= U * q["S"])).ravel())
        near = np.concatenate(near)
        assert not big or near.mean() >= 1e-3, float(near.mean())
    elif family == "offset":
        q = _direction(flow, image, 3, 2, "exponential", alpha, 0.0)
        assert np.median(np.abs(flow.astype(np.float64)[:, :, :, :W - 2]) / np.maximum(q["S"], 2.0 ** -149)) > 1e5
    elif family == "graded":
        top = np.abs(flow.astype(np.float64)).max(axis=(0, 1, 2))
        for b, e in enumerate(GRADED_EXPONENTS[:-(-W // GRADED_BAND)]):
            m = top[b * GRADED_BAND:(b + 1) * GRADED_BAND].max()
            assert 2.0 ** (e - 4) <= m < 2.0 ** e, (e, m)
    elif family == "alpha0":
        assert float(np.float32(alpha)) == 0.0 and np.ptp(image) > 0.5
        for edge in EDGES:
            assert (_direction(flow, image, 3, 1, edge, alpha, 0.0)["w"] == 1.0).all()


# ------------------------------------------------------------------ the header's operation list in float32
def emulate(flow, image, go, order=1, edge="exponential", alpha=150.0, eps=0.001, mutate=None):
    """(out, grad_flow) in float32, following include/flownet2_hip_smooth.h operation by operation in numpy float32 (every
    operation rounded on its own): sqrt and rsq correctly rounded, exp2 correctly rounded and then flushed to 0 below 2^-126.
    ``mutate`` plants one mistake, for the tests that show which family catches it:
      "d2_regrouped"     the second difference formed as (f[x + 2] - 2 f[x + 1]) + f[x]
      "clamped_exponent" exp2's argument clamped at -125, so that no weight is below 2^-125 and none is flushed"""
    f32 = np.float32
    f, im, g = np.asarray(flow, f32), np.asarray(image, f32), np.asarray(go, f32)
    N, F, H, W = f.shape
    C, k = im.shape[1], order
    al, ep = f32(alpha), f32(eps)
    eps2 = f32(ep * ep)
    out, grad = np.zeros((N, 2, H, W), f32), np.zeros((N, F, H, W), f32)
    with np.errstate(under="ignore"):
        for plane, axis in ((0, 3), (1, 2)):
            L = f.shape[axis]
            if L <= k:
                continue
            t = al * (im[_sl(axis, k, L)] - im[_sl(axis, 0, L - k)])
            a = np.abs(t) if edge == "exponential" else t * t
            e = ((a[:, 0:1] + a[:, 1:2]) + a[:, 2:3]) * f32(1.0 / 3.0) if C == 3 else a
            arg = -(e * f32(1.44269504))
            if mutate == "clamped_exponent":
                arg = np.maximum(arg, f32(-125))
            w = np.exp2(arg.astype(np.float64)).astype(f32)
            w = np.where(w < f32(FLOOR), f32(0), w)
            if k == 1:
                d = f[_sl(axis, 1, L)] - f[_sl(axis, 0, L - 1)]
            elif mutate == "d2_regrouped":
                d = (f[_sl(axis, 2, L)] - f32(2) * f[_sl(axis, 1, L - 1)]) + f[_sl(axis, 0, L - 2)]
            else:
                d = (f[_sl(axis, 2, L)] - f[_sl(axis, 1, L - 1)]) - (f[_sl(axis, 1, L - 1)] - f[_sl(axis, 0, L - 2)])
            s = d * d + eps2
            if eps2 == 0:
                rho, drho = np.abs(d), np.sign(d)
            else:
                rho = np.sqrt(s)
                drho = d * (1.0 / np.sqrt(s.astype(np.float64))).astype(f32)
            acc = rho[:, 0:1]
            for c in range(1, F):
                acc = acc + rho[:, c:c + 1]
            prod = w * acc
            valid = (slice(None), slice(plane, plane + 1)) + _sl(axis, 0, L - k)[2:]
            out[valid] = prod
            tt = np.zeros((N, F, H, W), f32)      # t per cell, 0 where no cell is
            tt[_sl(axis, 0, L - k)] = (g[valid] * w) * drho
            pad = [(0, 0)] * 4
            pad[axis] = (2, 0)
            tp = np.pad(tt, pad)                  # tp[q + 2] = t[q]
            t0, t1, t2 = tp[_sl(axis, 2, L + 2)], tp[_sl(axis, 1, L + 1)], tp[_sl(axis, 0, L)]
            gdir = t1 - t0 if k == 1 else (t2 - f32(2) * t1) + t0
            grad = gdir if plane == 0 else grad + gdir
            if plane == 1 and W <= k:
                grad = gdir
    return out, grad


def dyadic_flow(shape, seed, patch=3):
    """N x F x H x W float32 of multiples of 1/8 with |f| <= 64, constant on patch x patch squares: every first and second
    difference is exact in fp32, and many are 0."""
    N, F, C, H, W = shape
    rng = np.random.default_rng(seed)
    coarse = rng.integers(-512, 513, (N, F, -(-H // patch), -(-W // patch))).astype(np.float32) / np.float32(8)
    return np.repeat(np.repeat(coarse, patch, axis=2), patch, axis=3)[:, :, :H, :W].copy()
