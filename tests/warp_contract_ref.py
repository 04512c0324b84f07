"""float64 references, per-element error bounds and input families for the float32 warp and norm kernels (csrc/resample2d.hip,
csrc/channelnorm.hip) -- TEST INFRASTRUCTURE ONLY, a helper module (not a conftest).  tests/test_warp_contract_host.py checks this
module against the oracle and against mutants of itself; tests/test_gpu_warp_contract.py checks the kernels against it.

THE POSITION is part of the contract and is formed exactly as the reference kernels form it, in fp32: xf = fl32(x + dx), floorf(xf),
the saturating float -> int conversions (NaN -> 0), the floored fraction fa = fl32(xf - floorf(xf)) the gathers use and the TRUNCATED
fraction ta = fl32(xf - (float)int(xf)) the scatter uses.  Both subtractions are exact in fp32 except fa for xf in (-1, 0), where
xf + 1 is rounded (and ta = xf is negative): there the rounded fp32 value IS the contract.  Everything after the position -- weights,
products, sums -- is float64 here and fp32 / double in the kernels, and the bounds below are the rounding error of the kernels'
operation sequence against it.  u = 2^-24 (round to nearest: every fp32 operation errs by at most u relative, or by 2^-150 absolute
where its result is subnormal).  Sums of n terms in any order err by at most (n - 1) u sum|terms| with no higher-order term (Jeannerod
& Rump 2013), so the first-order bounds below are rigorous.

  forward, bilinear   weights in double from fa / fb (their rounding, 2^-53, is noise), each of the n = 4 ks^2 terms (float)(w * i)
                      rounded once, fp32 chain from 0 (first add exact): n u sum|w i|; each rounding to a subnormal adds 2^-150:
                          delta = 4 ks^2 u sum|w i| + 4 ks^2 2^-149        (2^-147 at ks = 1)
                      This is the kernels' sequence.  The reference and the oracle round the BR term twice (resample_fwd_seq32 tells
                      why): fl(alpha * beta) errs by u relative, or by 2^-150 where it underflows, so their bound is
                          delta_ref = delta + u sum|w11 i| + 2^-149 sum|i_BR|
                      and the host test holds the oracle to delta_ref, the kernels' sequence in numpy to delta.
  forward, nearest    an exact copy: delta = 0
  grad_flow           per channel and window offset four terms (g * go) * i with g = gam = fl(1 - fa) or fl(1 - gam): each g errs by at
                      most u ABSOLUTELY (two roundings of values in [0, 1], u / 2 each) -- not relative to a small weight, so the bound
                      uses unweighted terms |go| |i|: u for g, 2 u for the two products, n u for the chain of n = 4 C (span + 1)^2
                      <= 4 C ks^2 adds:
                          delta = (4 C ks^2 + 4) u sum|go| |i_corner| + 2^-150 sum(1 + |i_corner|)
                      (the floor: an underflowing g * go errs by 2^-150, times |i|; an underflowing product by 2^-150)
  grad_input1         a cell with N non-zero contributions t = w * go, w = fl(fl(1 - ta) * fl(1 - tb)) etc.: three roundings in the
                      weight, one in the product, at most N in the sum whatever its order or grouping (fp32 atomics, fp64 LDS cells
                      rounded once at the flush, the three-channel scatter); a non-zero prefill is one more term:
                          delta = (N + 4) u (sum|t| + |prefill|) + 2^-149 sum(1 + |go|)
                      (the floor: an underflowing weight product errs by 2^-150, times |go|; an underflowing t by 2^-150; doubled)
  ChannelNorm forward squares rounded (u), C - 1 adds of non-negative terms (u each): C u relative on the sum, half of it on the root,
                      plus the root's own rounding; a square that underflows errs by at most 2^-150, all C of them move the root by at
                      most sqrt(C 2^-150):
                          delta = (C / 2 + 1.5) u ref + sqrt(C) 2^-74
  ChannelNorm backward (float)((double)fl(go * x) / ((double)out + 1e-9)) with `out` as the kernel produced it: the product and the
                      final conversion round (the double division's 2^-53 is inside the margin of 2 u against u / (1 + u) each); a
                      product that underflows errs by 2^-150 before the division:
                          delta = 2 u |ref| + 2^-149 + 2^-150 / (out + 1e-9)

WILD pixels -- a non-finite flow component, or |xf| or |yf| >= 2^31 -- have no float64 bound ((float)int(xf) saturates, the weights
overflow, fp32 overflow depends on the summation order): their forward and grad_flow values are compared with the oracle bit for bit,
and the grad_input1 cells they touch (their clamped corners) are excluded.  Excluded cells are a condition of a case, at most
EXCLUDED_CAP of its cells; the `wild` family places its pixels under that cap by construction."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from lowp_ref import bracket, outside
from resample_det_ref import f2i_sat

U = 2.0 ** -24
F32, F64 = np.float32, np.float64
TW, R = 64, 16                      # tile width and window margin of every tiled kernel
EXCLUDED_CAP = 0.05
INT_MIN, INT_MAX = -2147483648, 2147483647


# ------------------------------------------------------------------ the kernels' host-side choices, restated
def tile_height(B, H, tiles_x):
    """tile_height() of csrc/resample2d.hip: the height that needs fewer window rows over all rounds of 512 resident tiles."""
    t32, t48 = B * tiles_x * ((H + 31) // 32), B * tiles_x * ((H + 47) // 48)
    c32, c48 = ((t32 + 511) // 512) * (32 + 32), ((t48 + 511) // 512) * (48 + 32)
    return 48 if c48 < c32 else 32


def tileable(Hi, Wi, H, W):
    """tiled_shape_ok() for a dense, 16-byte aligned image."""
    return Hi == H and Wi == W and W % 4 == 0 and H >= 16 and W >= 32


def sample_pixels(H, W, TH=32):
    """(x, y) of the four pixels per tile whose flow places the backward windows (tile_flow_sample): {(ty, tx): [(x, y)] * 4}."""
    out = {}
    for ty in range((H + TH - 1) // TH):
        for tx in range((W + TW - 1) // TW):
            out[(ty, tx)] = [(min(tx * TW + TW // 4 + (q & 1) * (TW // 2), W - 1), min(ty * TH + TH // 4 + (q >> 1) * (TH // 2), H - 1))
                             for q in range(4)]
    return out


# ------------------------------------------------------------------ positions
def d2i_sat(v):
    """the saturating double -> int conversion (truncation; NaN -> 0)."""
    v = np.asarray(v, F64)
    return np.trunc(np.where(np.isnan(v), 0.0, np.clip(v, INT_MIN, INT_MAX))).astype(np.int64)


def pos_core(xs, ys, dx, dy, mut=()):
    """The position of pixels (xs, ys) with flow (dx, dy), arrays of one shape: everything the kernels derive in fp32 before a clamp."""
    with np.errstate(all="ignore"):
        xf = (xs.astype(F32) + dx.astype(F32)).astype(F32)
        yf = (ys.astype(F32) + dy.astype(F32)).astype(F32)
        fx, fy = np.floor(xf), np.floor(yf)
        one = F32(1)
        P = SimpleNamespace(xf=xf, yf=yf)
        P.ixL, P.ixR = f2i_sat(fx), f2i_sat((fx + one).astype(F32))
        P.iyT, P.iyB = f2i_sat(fy), f2i_sat((fy + one).astype(F32))
        P.fa, P.fb = (xf - fx).astype(F32), (yf - fy).astype(F32)                  # floored: forward and grad_flow
        P.ta = (xf - f2i_sat(xf).astype(F32)).astype(F32)                          # truncated: the scatter
        P.tb = (yf - f2i_sat(yf).astype(F32)).astype(F32)
        if "floor_scatter" in mut:
            P.ta, P.tb = P.fa, P.fb
        if "rint" in mut:
            P.nx, P.ny = d2i_sat(np.rint(xf.astype(F64))), d2i_sat(np.rint(yf.astype(F64)))
        else:
            P.nx, P.ny = d2i_sat(np.floor(xf.astype(F64) + 0.5)), d2i_sat(np.floor(yf.astype(F64) + 0.5))
        P.wild = ~(np.isfinite(dx) & np.isfinite(dy) & (np.abs(xf.astype(F64)) < 2.0 ** 31) & (np.abs(yf.astype(F64)) < 2.0 ** 31))
    return P


def positions(flow, mut=()):
    flow = np.asarray(flow, F32)
    B, _, H, W = flow.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return pos_core(np.broadcast_to(xs, (B, H, W)), np.broadcast_to(ys, (B, H, W)), flow[:, 0], flow[:, 1], mut)


def _gather_corners(P, b, H, W, Hi, Wi, mut):
    """the gathers' corners before the window shift: clamped with the FLOW dims (the image dims follow with the shift)"""
    if "image_clamp" in mut:
        return P.ixL[b], P.ixR[b], P.iyT[b], P.iyB[b]
    return np.clip(P.ixL[b], 0, W - 1), np.clip(P.ixR[b], 0, W - 1), np.clip(P.iyT[b], 0, H - 1), np.clip(P.iyB[b], 0, H - 1)


def _scatter_cells(P, sel, Hi, Wi, ks):
    """flat cell indices of the scatter corners of the pixels `sel` selects (any index), every window offset: list of arrays"""
    xL, xR = np.clip(P.ixL[sel], 0, Wi - 1), np.clip(P.ixR[sel], 0, Wi - 1)
    yT, yB = np.clip(P.iyT[sel], 0, Hi - 1), np.clip(P.iyB[sel], 0, Hi - 1)
    out = []
    for ky in range(ks):
        for kx in range(ks):
            yt, yb = np.clip(yT + ky, 0, Hi - 1), np.clip(yB + ky, 0, Hi - 1)
            xl, xr = np.clip(xL + kx, 0, Wi - 1), np.clip(xR + kx, 0, Wi - 1)
            out += [yt * Wi + xl, yt * Wi + xr, yb * Wi + xl, yb * Wi + xr]
    return out


def excluded_cells(flow, Hi, Wi, ks=1):
    """B x Hi x Wi mask of the grad_input1 cells wild pixels touch (the same in every channel)."""
    P = positions(flow)
    B = P.wild.shape[0]
    ex = np.zeros((B, Hi * Wi), bool)
    for b in range(B):
        Pb = SimpleNamespace(ixL=P.ixL[b], ixR=P.ixR[b], iyT=P.iyT[b], iyB=P.iyB[b])
        for cells in _scatter_cells(Pb, P.wild[b], Hi, Wi, ks):
            ex[b, cells] = True
    return ex.reshape(B, Hi, Wi)


# ------------------------------------------------------------------ references
def resample_fwd64(img, flow, ks=1, bilinear=True, mut=(), br_twice=False):
    """(ref, delta, wild): Resample2d forward in float64 from the fp32 position, its bound, the B x H x W mask of wild pixels.
    br_twice: the bound of the REFERENCE's sequence (the oracle's) instead of the kernels' -- its BR term is fl(fl(alpha * beta) * i), one
    more fp32 rounding on that term: u |w11 i| more (2^-149 |i| where alpha * beta underflows)."""
    img, flow = np.asarray(img, F32), np.asarray(flow, F32)
    B, C, Hi, Wi = img.shape
    _, _, H, W = flow.shape
    P = positions(flow, mut)
    ref, absr, extra = np.zeros((B, C, H, W)), np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    with np.errstate(all="ignore"):
        for b in range(B):
            I = img[(b + 1) % B if "batch" in mut else b].astype(F64)
            if not bilinear:                                   # nearest ignores kernel_size
                xN = np.clip(np.clip(P.nx[b], 0, W - 1), 0, Wi - 1)
                yN = np.clip(np.clip(P.ny[b], 0, H - 1), 0, Hi - 1)
                ref[b] = I[:, yN, xN]
                continue
            a, be = P.fa[b].astype(F64), P.fb[b].astype(F64)
            w = [(1 - a) * (1 - be), a * (1 - be), (1 - a) * be, a * be]
            xL, xR, yT, yB = _gather_corners(P, b, H, W, Hi, Wi, mut)
            for ky in range(ks):
                for kx in range(ks):
                    yt, yb = np.clip(yT + ky, 0, Hi - 1), np.clip(yB + ky, 0, Hi - 1)
                    xl, xr = np.clip(xL + kx, 0, Wi - 1), np.clip(xR + kx, 0, Wi - 1)
                    for wk, (yy, xx) in zip(w, ((yt, xl), (yt, xr), (yb, xl), (yb, xr))):
                        t = wk * I[:, yy, xx]
                        ref[b] += t
                        absr[b] += np.abs(t)
                    extra[b] += U * np.abs(t) + 2.0 ** -149 * np.abs(I[:, yb, xr])          # t: the BR term
    n = 4 * ks * ks
    delta = n * U * absr + n * 2.0 ** -149 if bilinear else np.zeros_like(absr)
    if br_twice and bilinear:
        delta = delta + extra
    return ref, delta, P.wild


def resample_fwd_seq32(img, flow, ks=1):
    """(out, br_zero): the bilinear forward with the HIP kernels' documented operation sequence, operation by operation in numpy --
    all four weights in double from fa / fb, every term (float)(w * (double)i) rounded once, one fp32 chain from 0 over the window
    offsets in the order TL, TR, BL, BR -- and the mask of elements whose every BR term is exactly zero.  The kernels must have these
    bits.  The reference (resample2d_kernel.cu:59) and the oracle form the BR term `(alpha) * (beta) * I` without a double literal,
    i.e. in fp32 with two roundings, where the kernels use the double product a * be like the other three: the two agree bit for
    bit exactly where the BR terms vanish or round alike."""
    img, flow = np.asarray(img, F32), np.asarray(flow, F32)
    B, C, Hi, Wi = img.shape
    _, _, H, W = flow.shape
    P = positions(flow)
    out, br_zero = np.zeros((B, C, H, W), F32), np.ones((B, C, H, W), bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            I = img[b].astype(F64)
            a, be = P.fa[b].astype(F64), P.fb[b].astype(F64)
            w = [(1 - a) * (1 - be), a * (1 - be), (1 - a) * be, a * be]
            xL, xR, yT, yB = _gather_corners(P, b, H, W, Hi, Wi, ())
            for ky in range(ks):
                for kx in range(ks):
                    yt, yb = np.clip(yT + ky, 0, Hi - 1), np.clip(yB + ky, 0, Hi - 1)
                    xl, xr = np.clip(xL + kx, 0, Wi - 1), np.clip(xR + kx, 0, Wi - 1)
                    for k, (yy, xx) in enumerate(((yt, xl), (yt, xr), (yb, xl), (yb, xr))):
                        t = (w[k] * I[:, yy, xx]).astype(F32)
                        out[b] = (out[b] + t).astype(F32)
                        if k == 3:
                            br_zero[b] &= ~(t != 0)          # (a NaN term is not zero)
    return out, br_zero


def resample_bwd64(img, flow, gout, ks=1, mut=(), prefill=None):
    """Resample2d backward in float64 from the fp32 position: a namespace with gimg, gimg_delta (B x C x Hi x Wi), gflow, gflow_delta
    (B x 2 x H x W), the sums of absolute terms the bounds are made of (gimg_abs, gimg_n, gflow_abs), wild (B x H x W), excluded (B x Hi x Wi:
    cells wild pixels touch) and reached (B x C x Hi x Wi: cells with a non-zero contribution).  Wild pixels contribute nothing here."""
    img, flow, gout = np.asarray(img, F32), np.asarray(flow, F32), np.asarray(gout, F32)
    B, C, Hi, Wi = img.shape
    _, _, H, W = flow.shape
    P = positions(flow, mut)
    n = Hi * Wi
    pre = np.zeros((B, C, n)) if prefill is None else np.asarray(prefill, F64).reshape(B, C, n)
    gimg, gabs, gcnt, gfloor = pre.copy(), np.abs(pre), (pre != 0).astype(F64), np.zeros((B, C, n))
    gflow, fabs, ffloor = np.zeros((B, 2, H, W)), np.zeros((B, H, W)), np.zeros((B, H, W))
    span = 2 * ((ks - 1) // 2)
    with np.errstate(all="ignore"):
        for b in range(B):
            ok = ~P.wild[b]
            I = img[(b + 1) % B if "batch" in mut else b].astype(F64)
            go = np.where(ok[None], gout[b].astype(F64), 0.0)
            # ---- grad_input1: truncated fractions, corners clamped with the image dims
            a, be = np.where(ok, P.ta[b].astype(F64), 0.0), np.where(ok, P.tb[b].astype(F64), 0.0)
            w = [(1 - a) * (1 - be), a * (1 - be), (1 - a) * be, a * be]
            Pb = SimpleNamespace(ixL=P.ixL[b], ixR=P.ixR[b], iyT=P.iyT[b], iyB=P.iyB[b])
            for k, cells in enumerate(_scatter_cells(Pb, slice(None), Hi, Wi, ks)):
                cf = cells.ravel()
                for c in range(C):
                    t = (w[k % 4] * go[c]).ravel()
                    nz = (t != 0).astype(F64)
                    gimg[b, c] += np.bincount(cf, weights=t, minlength=n)
                    gabs[b, c] += np.bincount(cf, weights=np.abs(t), minlength=n)
                    gcnt[b, c] += np.bincount(cf, weights=nz, minlength=n)
                    gfloor[b, c] += np.bincount(cf, weights=nz * (1 + np.abs(go[c].ravel())), minlength=n)
            # ---- grad_flow: floored fractions, corners clamped with the flow dims, then shifted and clamped to the image
            gam_y, gam_x = 1 - P.fa[b].astype(F64), 1 - P.fb[b].astype(F64)
            xL, xR, yT, yB = _gather_corners(P, b, H, W, Hi, Wi, mut)
            for i in range(span + 1):
                for j in range(span + 1):
                    yt, yb = np.clip(yT + j, 0, Hi - 1), np.clip(yB + j, 0, Hi - 1)
                    xl, xr = np.clip(xL + i, 0, Wi - 1), np.clip(xR + i, 0, Wi - 1)
                    iTL, iTR, iBL, iBR = I[:, yt, xl], I[:, yt, xr], I[:, yb, xl], I[:, yb, xr]
                    dBR = 0.0 if "drop" in mut else (1 - gam_y) * go * iBR
                    gflow[b, 1] += (gam_y * go * iBL - gam_y * go * iTL + dBR - (1 - gam_y) * go * iTR).sum(0)
                    gflow[b, 0] += (gam_x * go * iTR - gam_x * go * iTL + (1 - gam_x) * go * iBR - (1 - gam_x) * go * iBL).sum(0)
                    s = np.abs(iTL) + np.abs(iTR) + np.abs(iBL) + np.abs(iBR)
                    fabs[b] += (np.abs(go) * s).sum(0)
                    ffloor[b] += (4 + s).sum(0)
    r = SimpleNamespace(wild=P.wild, excluded=excluded_cells(flow, Hi, Wi, ks))
    r.gimg, r.gimg_abs, r.gimg_n = (v.reshape(B, C, Hi, Wi) for v in (gimg, gabs, gcnt))
    r.reached = (gcnt - (pre != 0)).reshape(B, C, Hi, Wi) > 0
    r.gimg_delta = (r.gimg_n + 4) * U * r.gimg_abs + 2.0 ** -149 * gfloor.reshape(B, C, Hi, Wi)
    r.gflow, r.gflow_abs = gflow, fabs
    d = (4 * C * ks * ks + 4) * U * fabs + 2.0 ** -150 * ffloor
    r.gflow_delta = np.stack((d, d), axis=1)
    return r


def chnorm_fwd64(x):
    """(ref, delta) of ChannelNorm forward on float32 x."""
    C = x.shape[1]
    ref = np.sqrt((np.asarray(x, F32).astype(F64) ** 2).sum(1, keepdims=True))
    return ref, (C / 2 + 1.5) * U * ref + np.sqrt(C) * 2.0 ** -74


def chnorm_bwd64(x, out, go):
    """(ref, delta) of ChannelNorm backward; `out` (B x 1 x H x W) as the kernel produced it, `go` of the same shape."""
    den = np.asarray(out, F32).astype(F64) + 1e-9
    ref = np.asarray(go, F32).astype(F64) * np.asarray(x, F32).astype(F64) / den
    return ref, 2 * U * np.abs(ref) + 2.0 ** -149 + 2.0 ** -150 / den + np.zeros_like(ref)


# ------------------------------------------------------------------ comparing
def ratio_and_check(got, ref, delta, ok=None, what=""):
    """Asserts that every element of `got` (fp32) selected by `ok` lies in bracket(ref, delta) (lowp_ref: widened by delta, rounded
    outward to fp32); returns the worst |got - ref| / delta (0 where delta is 0 and the values agree)."""
    got = np.asarray(got, F32)
    ok = np.ones(got.shape, bool) if ok is None else np.broadcast_to(ok, got.shape)
    g = np.where(ok, got, F32(0))
    r, d = np.where(ok, ref, 0.0), np.where(ok, delta, 0.0)
    lo, hi = bracket(torch.from_numpy(r), torch.from_numpy(d), torch.float32)
    bad = outside(torch.from_numpy(g), lo, hi).numpy()
    with np.errstate(all="ignore"):
        err = np.abs(g.astype(F64) - r)
        ratio = np.where(err == 0, 0.0, err / d)
    if bad.any():
        i = np.unravel_index(int(np.flatnonzero(bad)[0]), got.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(ok.sum())} elements outside the bracket; first at {i}: got {g[i]!r}, "
                             f"ref {r[i]!r} +- {d[i]!r} (err / delta = {ratio[i]:.3g})")
    ratio = np.where(np.isfinite(ratio), ratio, 0.0)      # err inside the outward fp32 rounding of a zero-width bracket
    return float(ratio.max()) if ratio.size else 0.0


def same_bits(a, b):
    """elementwise: the same fp32 bits, or NaN in both (payloads and signs of NaN are not part of the contract)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulp_distance(a, b):
    """worst distance in units of fp32 representable values over the elements that are not NaN in either"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    m = ~(np.isnan(a) | np.isnan(b))
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, INT_MIN - ia, ia), np.where(ib < 0, INT_MIN - ib, ib)
    return int(np.abs(ia - ib)[m].max()) if m.any() else 0


# ------------------------------------------------------------------ image and grad_out families
def graded(shape, seed):
    """full 24-bit mantissas, random signs; plane (b, c) scaled by a power of two of its own within 2^+-24; one plane all zero: a read
    from the wrong batch item or channel leaves every bracket."""
    B, C = shape[:2]
    rng = np.random.default_rng(1000 + seed)
    m = rng.integers(2 ** 23, 2 ** 24, shape).astype(F64) * 2.0 ** -23 * rng.choice([-1.0, 1.0], shape)
    n = B * C
    e = rng.permutation(np.round(np.linspace(-24, 24, n)).astype(int)) if n > 1 else np.zeros(1, int)
    out = m * (2.0 ** e.astype(F64)).reshape(B, C, *([1] * (len(shape) - 2)))
    if n > 1:
        out.reshape(n, -1)[seed % n] = 0.0
    return out.astype(F32)


def unit(shape, seed):
    return (np.random.default_rng(2000 + seed).random(shape) - 0.5).astype(F32)


IMAGES = {"graded": graded, "unit": unit}


def chnorm_input(shape):
    """ChannelNorm's input: graded planes, none of them all zero (the dropped leading channel holds that one), one pixel exactly zero"""
    B, C, H, W = shape
    x = np.ascontiguousarray(graded((B, C + 1, H, W), 0)[:, 1:])
    x[0, :, 0, 0] = 0
    return x


# ------------------------------------------------------------------ flow families
def _coords(B, H, W):
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    idx = np.arange(B * H * W).reshape(B, H, W)
    return np.broadcast_to(xs, (B, H, W)), np.broadcast_to(ys, (B, H, W)), idx


def _to_flow(tx, ty, xs, ys):
    """the flow that sends pixel (xs, ys) to the fp32 targets (tx, ty): target - coordinate, formed in double, rounded once"""
    return np.stack(((tx.astype(F64) - xs).astype(F32), (ty.astype(F64) - ys).astype(F32)), axis=1)


def _up(v):
    return np.nextafter(np.asarray(v, F32), F32(np.inf))


def _down(v):
    return np.nextafter(np.asarray(v, F32), F32(-np.inf))


def noise(B, H, W, seed=0, **_):
    """today's family: sigma = 4 px, 1 % of the values times 20"""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((B, 2, H, W)) * 4.0).astype(F32)
    f.reshape(-1)[rng.integers(0, f.size, f.size // 100)] *= F32(20.0)
    return f


def _grid_axis(coord, k):
    """per pixel: target n + f with n = k % 5 - 2 around the pixel's own coordinate and fraction kind k // 5 (0 .. 8); returns the
    flow component"""
    base = (coord + (k % 5 - 2)).astype(F32)
    kind = k // 5
    t = base.copy()
    t = np.where(kind == 1, np.where(base == 0, F32(2.0 ** -24), _up(base)), t)     # the smallest fraction: 2^-24 at 0, else one ulp
    t = np.where(kind == 2, _down(base + F32(0.5)), t)
    t = np.where(kind == 3, base + F32(0.5), t)
    t = np.where(kind == 4, _up(base + F32(0.5)), t)
    t = np.where(kind == 5, _down(base + F32(1)), t)
    t = np.where(kind == 8, F32(-0.05) - F32(0.9) * ((k % 5) / F32(5)).astype(F32), t)      # a target in (-1, 0)
    d = (t.astype(F64) - coord).astype(F32)
    d = np.where(kind == 6, F32(-2.0 ** -25), d)                                   # xf rounds back to x (x >= 1), -2^-25 at x = 0
    d = np.where(kind == 7, F32(-0.0), d)
    return d


def grid(B, H, W, seed=0, **_):
    """every pixel targets n + f: n in -2 .. 2 around its own position, f in {0, smallest, 0.5 - ulp, 0.5, 0.5 + ulp, 1 - ulp}; also
    dx = -2^-25, dx = -0.0 and targets in (-1, 0); the x and y kinds run through all 45 x 45 combinations with the pixel index"""
    xs, ys, idx = _coords(B, H, W)
    idx = idx + 17 * seed
    return np.stack((_grid_axis(xs, idx % 45), _grid_axis(ys, (idx * 7 + idx // 45 + 3) % 45)), axis=1)


def _border_targets(n, ni):
    t = [F32(-1), F32(-0.5), _down(F32(0)), F32(0), F32(n - 1), _up(F32(n - 1)), F32(n - 0.5), F32(n)]
    if ni != n:
        t += [F32(ni - 1), _up(F32(ni - 1)), F32(ni - 0.5), F32(ni)]
    return np.array(t, F32)


def border(B, H, W, Hi=None, Wi=None, seed=0, **_):
    """pixels target exactly -1, -0.5, -ulp, 0, W - 1, W - 1 + ulp, W - 0.5, W (and the same with Wi where it differs) in x, the same
    with H (Hi) in y, in all combinations; every fifth pixel keeps its own column, another fifth its own row instead"""
    xs, ys, idx = _coords(B, H, W)
    idx = idx + 5 * seed
    Tx, Ty = _border_targets(W, Wi or W), _border_targets(H, Hi or H)
    tx = np.where(idx % 5 == 1, xs.astype(F32), Tx[idx % len(Tx)])
    ty = np.where(idx % 5 == 3, ys.astype(F32), Ty[(idx * 7 + idx // len(Tx) + 1) % len(Ty)])
    return _to_flow(tx, ty, xs, ys)


def _window_axis(coord, T0, TT, k):
    """targets just outside, on and just inside both edges of the window [T0 - R, T0 + TT + R - 1] of a tile starting at T0, or
    (k == 6) the own coordinate"""
    lo, hi = (T0 - R).astype(F32), (T0 + TT + R - 1).astype(F32)
    t = coord.astype(F32)
    for kind, v in enumerate((lo - F32(1), lo, _up(lo), _down(hi), hi, hi + F32(1))):
        t = np.where(k == kind, v, t)
    return t


def window(B, H, W, TH=32, seed=0, **_):
    """per TH x 64 tile with R = 16: pixels target the column and row just outside, on and just inside each of the four window edges
    (the in-window test of the tiled kernels); the four sample pixels have zero flow, so the backward window stays on the tile"""
    xs, ys, idx = _coords(B, H, W)
    idx = idx + 3 * seed
    tx = _window_axis(xs, xs // TW * TW, TW, idx % 7)
    ty = _window_axis(ys, ys // TH * TH, TH, (idx * 3 + idx // 7 + 2) % 7)
    f = _to_flow(tx, ty, xs, ys)
    for pts in sample_pixels(H, W, TH).values():
        for x, y in pts:
            f[:, :, y, x] = 0.0
    return f


TRANSLATIONS = (7.9, 8.0, 8.1, -8.0, 13.9, 24.0, -24.0, 40.0, 999999.0, 1.0e6, 1.1e6)
OUTLIERS = (np.nan, np.inf, 1.0e30)
N_SETTINGS = 6
FOLLOW_TABLE = len(TRANSLATIONS) * 3 * N_SETTINGS      # 198 tiles hold every translation x direction x setting once
FOLLOW_STEP = 66                                       # tiles of one FOLLOW_WIDE case: seeds 0, 1, 2 walk the table


def follow_plan(b, ty, tx, tiles_y, tiles_x, seed):
    """(translation, direction, sample-pixel setting, rotation) of one tile: direction 0 = x, 1 = y, 2 = both.  The tile's running
    index (plus FOLLOW_STEP per seed) is decomposed in mixed radix, so FOLLOW_TABLE consecutive indices are the whole table
    translation x direction x setting, each entry once."""
    k = (b * tiles_y + ty) * tiles_x + tx + FOLLOW_STEP * seed
    return TRANSLATIONS[k % 11], (k // 11) % 3, (k // 33) % N_SETTINGS, (k + k // 11 + k // 33) % 4


def follow(B, H, W, TH=32, seed=0, **_):
    """per tile a constant translation plus sigma = 1 noise, with the tile's four sample pixels set explicitly: 0 all agree, 1 one
    outlier (NaN, inf, 1e30), 2 two outliers, 3 the middle pair 7.9 px apart, 4 the middle pair 8.1 px apart, 5 left as noise"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((B, 2, H, W)).astype(F32)
    S = sample_pixels(H, W, TH)
    tiles_y, tiles_x = (H + TH - 1) // TH, (W + TW - 1) // TW
    for b in range(B):
        for (ty, tx), pts in S.items():
            T, direc, setting, rot = follow_plan(b, ty, tx, tiles_y, tiles_x, seed)
            for comp in (0, 1):
                tc = F32(T) if direc == 2 or direc == comp else F32(0)
                f[b, comp, ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW] += tc
                if setting == 0:
                    vals = [tc] * 4
                elif setting == 1:
                    vals = [tc] * 4
                    vals[rot] = F32(OUTLIERS[(rot + comp) % 3])
                elif setting == 2:
                    vals = [tc] * 4
                    vals[rot], vals[(rot + 1) % 4] = F32(OUTLIERS[(rot + comp) % 3]), F32(-1.0e30)
                elif setting in (3, 4):
                    vals = [tc - F32(20), tc, tc + F32(7.9 if setting == 3 else 8.1), tc + F32(30)]
                    vals = vals[rot:] + vals[:rot]
                else:
                    continue
                for q, (x, y) in enumerate(pts):
                    f[b, comp, y, x] = vals[q]
    return f


WILD_VALUES = (np.nan, np.inf, -np.inf, 1.0e30, -1.0e30, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 128, -(2.0 ** 31 - 128), 2.0 ** 24, -2.0 ** 24,
               2.0 ** 23 + 0.5, -(2.0 ** 23 + 0.5))


def wild(B, H, W, Hi=None, Wi=None, ks=1, TH=32, seed=0, **_):
    """`noise` with at most 2 % of the pixels (at least one) replaced by NaN, +-inf, +-1e30, +-2^31, +-(2^31 - 128), +-2^24,
    +-(2^23 + 0.5): dx only, dy only and both in turn, sample pixels of the tiles first.  A replacement whose cells would take the
    excluded share of grad_input1 past EXCLUDED_CAP is skipped, so the cap holds by construction."""
    Hi, Wi = Hi or H, Wi or W
    f = noise(B, H, W, seed)
    rng = np.random.default_rng(seed + 77)
    want = max(1, int(0.02 * B * H * W))
    cand = [(b, y, x) for b in range(B) for pts in sample_pixels(H, W, TH).values() for x, y in pts][:want // 2]
    cand += [(int(rng.integers(B)), int(rng.integers(H)), int(rng.integers(W))) for _ in range(4 * want)]
    budget = int(EXCLUDED_CAP * B * Hi * Wi)
    excl, done = set(), 0
    for j, (b, y, x) in enumerate(cand):
        if done >= want:
            break
        vals = WILD_VALUES[:7] if done == 0 else WILD_VALUES        # the first one is wild by the definition above in any case
        v = F32(vals[(j + seed + H + ks) % len(vals)])
        mode = (j + seed + W) % 3
        dx = v if mode != 1 else f[b, 0, y, x]
        dy = v if mode != 0 else f[b, 1, y, x]
        P = pos_core(np.array([x]), np.array([y]), np.array([dx], F32), np.array([dy], F32))
        new = set()
        if P.wild[0]:
            new = {(b, int(c[0])) for c in _scatter_cells(P, slice(None), Hi, Wi, ks)}
        if len(excl | new) > budget:
            continue
        excl |= new
        f[b, 0, y, x], f[b, 1, y, x] = dx, dy
        done += 1
    return f


FLOWS = {"noise": noise, "grid": grid, "border": border, "window": window, "follow": follow, "wild": wild}


# ------------------------------------------------------------------ the cases both test files use
class Case:
    """One (shape, kernel_size, flow family, seed): inputs and references are built once and shared (leave them unchanged)."""

    def __init__(self, img_shape, flow_hw=None, ks=1, family="noise", seed=0, backward=True, TH=None):
        self.img_shape, self.ks, self.family, self.seed, self.backward = tuple(img_shape), ks, family, seed, backward
        B, C, Hi, Wi = img_shape
        self.H, self.W = flow_hw or (Hi, Wi)
        self.TH = TH or 32
        self.id = f"{B}x{C}x{Hi}x{Wi}" + (f"-flow{self.H}x{self.W}" if flow_hw else "") + (f"-ks{ks}" if ks != 1 else "") + \
            f"-{family}{seed}"
        self.cache = {}      # results computed once per case: the references here, the oracle's outputs (the tests put them in)

    def cached(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    @property
    def tiled(self):
        B, C, Hi, Wi = self.img_shape
        return self.ks == 1 and tileable(Hi, Wi, self.H, self.W)

    @functools.cached_property
    def flow(self):
        B, C, Hi, Wi = self.img_shape
        return FLOWS[self.family](B, self.H, self.W, Hi=Hi, Wi=Wi, ks=self.ks, TH=self.TH, seed=self.seed)

    @functools.cached_property
    def img(self):
        return IMAGES["unit" if self.family == "noise" else "graded"](self.img_shape, self.seed)

    @functools.cached_property
    def gout(self):
        B, C = self.img_shape[:2]
        return IMAGES["unit" if self.family == "noise" else "graded"]((B, C, self.H, self.W), self.seed + 1)

    @functools.cached_property
    def prefill(self):
        p = graded(self.img_shape, self.seed + 2)
        return np.where(p == 0, F32(0), p)          # no -0.0: an added +0.0 would change its bits

    def excluded_share(self):
        B, C, Hi, Wi = self.img_shape
        return float(excluded_cells(self.flow, Hi, Wi, self.ks).mean())

    def fwd64(self, bilinear):
        return self.cached(("fwd64", bilinear), lambda: resample_fwd64(self.img, self.flow, self.ks, bilinear))

    @functools.cached_property
    def seq32(self):
        return resample_fwd_seq32(self.img, self.flow, self.ks)

    def bwd64(self, with_prefill):
        return self.cached(("bwd64", with_prefill), lambda: resample_bwd64(self.img, self.flow, self.gout, self.ks,
                                                                           prefill=self.prefill if with_prefill else None))


UNTILED_SHAPES = [((2, 3, 5, 7), None), ((2, 3, 9, 13), (6, 11)), ((2, 2, 6, 9), (9, 13)), ((2, 3, 8, 36), None), ((2, 1, 15, 32), None)]
TILED_SHAPES = [(2, 2, 16, 32), (2, 1, 33, 68), (1, 4, 35, 132), (1, 3, 16, 32), (2, 3, 33, 68), (1, 3, 35, 132)]
KS_SHAPES = [(2, 2, 9, 13), (1, 3, 16, 32)]
BIG_SHAPE = (1, 2, 96, 10944)          # tile_height() == 48 and C != 3: resample_fwd_tiled<48, ..., FUSE 0>; forward only
# one row of FOLLOW_STEP = 66 whole tiles (four distinct sample pixels each); with seeds 0, 1, 2 every entry of the table translation x
# direction x sample-pixel setting lands on one of them, for C = 3 (resample_bwd_c3x) and C != 3 (resample_bwd_tiled) separately
FOLLOW_WIDE = [(1, 2, 32, 64 * FOLLOW_STEP), (1, 3, 32, 64 * FOLLOW_STEP)]


def _cases():
    out = []
    for shape, fhw in UNTILED_SHAPES:
        out += [Case(shape, fhw, 1, fam) for fam in ("noise", "grid", "border", "wild")]
    for shape in TILED_SHAPES:
        out += [Case(shape, None, 1, fam) for fam in ("noise", "grid", "border", "window", "follow", "wild")]
        out += [Case(shape, None, 1, "follow", seed=1)]
    for shape in FOLLOW_WIDE:
        out += [Case(shape, None, 1, "follow", seed=s) for s in (0, 1, 2)]
    for shape in KS_SHAPES:
        out += [Case(shape, None, ks, fam) for ks in (2, 3) for fam in ("noise", "grid", "border", "wild")]
    out += [Case(BIG_SHAPE, None, 1, fam, backward=False, TH=48) for fam in ("noise", "window")]
    return out


CASES = _cases()
SMALL_CASES = [c for c in CASES if c.img_shape != BIG_SHAPE]
FUSED_SHAPES = [(2, 6, 33, 68), (1, 6, 16, 32), (2, 4, 17, 33)]          # B x 2C x H x W pairs
FUSED_CASES = [Case((B, C2 // 2, H, W), None, 1, fam) for B, C2, H, W in FUSED_SHAPES for fam in ("grid", "window", "follow", "wild")]


def branch(case):
    """the kernels a case reaches through the public entry points, for the reports"""
    B, C, Hi, Wi = case.img_shape
    if case.ks != 1:
        return "kernel_size > 1 (resample_fwd_ks_kernel / resample_bwd_ks_kernel)"
    if case.tiled:
        if C == 3:
            return "tiled, C = 3 (resample_fwd_tiled_all / resample_bwd_c3x)"
        if tile_height(B, case.H, (case.W + TW - 1) // TW) == 48:
            return "tiled, 48 rows (resample_fwd_tiled<48, FUSE 0>)"
        return "tiled, C != 3 (resample_fwd_tiled<32> / resample_bwd_tiled<32, ACC 1>)"
    return f"untiled (resample_fwd_kernel<{4 if case.W % 4 == 0 else 1}> / resample_bwd_kernel)"
CHNORM_SHAPES = [(2, 3, 16, 24), (1, 2, 7, 9), (3, 5, 6, 10)]
