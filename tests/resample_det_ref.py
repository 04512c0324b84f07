"""numpy restatement of the deterministic image gradient of Resample2d and WarpDiffNormCat (include/flownet2_hip.h,
fn2_resample2d_backward_det): per plane, fixed-point int64 sums of the fp32 contributions the atomic path adds, one
conversion to fp32, one fp32 add into the gradient; planes with an inf or a NaN are scattered serially in the oracle's order.
A helper module for the tests, not a conftest."""
import numpy as np

INF_BITS = 0x7F800000
INT_MAX, INT_MIN = 2147483647, -2147483648


def f2i_sat(v):
    """CUDA's saturating float -> int conversion (truncation; NaN -> 0), as the kernels and the oracle use it."""
    v = np.asarray(v, dtype=np.float32)
    d = v.astype(np.float64)
    out = np.trunc(np.where(np.isnan(d), 0.0, np.clip(d, INT_MIN, INT_MAX))).astype(np.int64)
    out = np.where(d >= 2147483520.0, INT_MAX, out)
    out = np.where(d <= -2147483648.0, INT_MIN, out)
    return out


def det_K(k, H, W):
    """The smallest K with 2^K >= 16 k^2 H W."""
    n, K = 16 * k * k * H * W, 0
    while (1 << K) < n:
        K += 1
    return K


def plane_max_bits(g):
    """max |g| of a plane as the bits of the fp32 magnitude (>= INF_BITS: inf or NaN in the plane)."""
    return int((np.ascontiguousarray(g, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)).max())


def exponent_E(m_bits):
    """2^(E-1) <= M < 2^E, subnormal M included (frexpf's exponent)."""
    if m_bits >= 0x00800000:
        return (m_bits >> 23) - 126
    return m_bits.bit_length() - 149


def plane_scale(g, K):
    """('zero', None), ('nonfinite', None) or ('finite', s) with s = 62 - E - K."""
    m = plane_max_bits(g)
    if m == 0:
        return "zero", None
    if m >= INF_BITS:
        return "nonfinite", None
    return "finite", 62 - exponent_E(m) - K


def scatter_geometry(flow_b, Hi, Wi, k):
    """The weights and target cells of every contribution of one batch item, in the oracle's order per pixel: a list over the window
    offsets (ky, kx) of four (weight, cell) pairs -- TL, TR, BL, BR -- with H x W arrays (fp32 weights, flat cell indices)."""
    _, H, W = flow_b.shape
    f32 = np.float32
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xf = xs.astype(f32) + flow_b[0].astype(f32)
    yf = ys.astype(f32) + flow_b[1].astype(f32)
    alpha = (xf - f2i_sat(xf).astype(f32)).astype(f32)          # truncation, not floor
    beta = (yf - f2i_sat(yf).astype(f32)).astype(f32)
    fx, fy = np.floor(xf), np.floor(yf)
    xL = np.clip(f2i_sat(fx), 0, Wi - 1)
    xR = np.clip(f2i_sat((fx + f32(1)).astype(f32)), 0, Wi - 1)
    yT = np.clip(f2i_sat(fy), 0, Hi - 1)
    yB = np.clip(f2i_sat((fy + f32(1)).astype(f32)), 0, Hi - 1)
    one = f32(1)
    w = [((one - alpha) * (one - beta)).astype(f32), (alpha * (one - beta)).astype(f32),
         ((one - alpha) * beta).astype(f32), (alpha * beta).astype(f32)]
    out = []
    for ky in range(k):
        for kx in range(k):
            yt, yb = np.clip(yT + ky, 0, Hi - 1), np.clip(yB + ky, 0, Hi - 1)
            xl, xr = np.clip(xL + kx, 0, Wi - 1), np.clip(xR + kx, 0, Wi - 1)
            out.append([(w[0], yt * Wi + xl), (w[1], yt * Wi + xr), (w[2], yb * Wi + xl), (w[3], yb * Wi + xr)])
    return out


def contributions(geom, g):
    """(v, cell) arrays of every contribution of one plane: v = fp32(weight * g)."""
    vs, cells = [], []
    for corners in geom:
        for w, cell in corners:
            vs.append((w * g.astype(np.float32)).astype(np.float32).ravel())
            cells.append(cell.ravel())
    return np.concatenate(vs), np.concatenate(cells)


def _int64_sums(q, cells, n):
    """exact per-cell sums of int64 values (two 32-bit halves summed in float64, exact below 2^21 terms per cell)."""
    hi = np.bincount(cells, weights=(q >> 32).astype(np.float64), minlength=n)
    lo = np.bincount(cells, weights=(q & 0xFFFFFFFF).astype(np.float64), minlength=n)
    return (hi.astype(np.int64) << 32) + lo.astype(np.int64)


def serial_scatter(geom, g, G):
    """The oracle's serial fp32 scatter into the flat plane G (in place): y, x, window offsets, corners TL TR BL BR."""
    H, W = g.shape
    for y in range(H):
        for x in range(W):
            for corners in geom:
                for w, cell in corners:
                    c = cell[y, x]
                    G[c] = np.float32(G[c] + np.float32(w[y, x] * g[y, x]))


def det_plane(geom, g, G, K, n):
    """Steps 1-6 for one plane: G (flat fp32, length n) is accumulated into in place."""
    kind, s = plane_scale(g, K)
    if kind == "zero":
        return
    if kind == "nonfinite":
        serial_scatter(geom, g, G)
        return
    v, cells = contributions(geom, g)
    q = np.rint(np.ldexp(v.astype(np.float64), s)).astype(np.int64)
    Q = _int64_sums(q, cells, n)
    r = np.ldexp(Q.astype(np.float64), -s).astype(np.float32)
    G[:] = (G + r).astype(np.float32)


def resample_bwd_det(img_shape, flow, gout, k=1, grad_init=None):
    """grad_input1 of the deterministic Resample2d backward: img_shape = (B, C, Hi, Wi), flow B x 2 x H x W, gout B x C x H x W; grad_init:
    the tensor accumulated into (zeros if None)."""
    B, C, Hi, Wi = img_shape
    _, _, H, W = gout.shape
    flow = np.asarray(flow, dtype=np.float32)
    gout = np.asarray(gout, dtype=np.float32)
    G = np.zeros((B, C, Hi * Wi), np.float32) if grad_init is None else np.array(grad_init, np.float32).reshape(B, C, Hi * Wi).copy()
    K = det_K(k, H, W)
    for b in range(B):
        geom = scatter_geometry(flow[b], Hi, Wi, k)
        for c in range(C):
            det_plane(geom, gout[b, c], G[b, c], K, Hi * Wi)
    return G.reshape(B, C, Hi, Wi)


def chnorm_grad(gn, diff, nrm):
    """channelnorm_kernel.cu:93 as the kernels evaluate it: fp32 product, double division, rounded to fp32."""
    prod = (gn * diff).astype(np.float32)
    return (prod.astype(np.float64) / (nrm.astype(np.float64) + 1e-9)).astype(np.float32)


def warped_grad(pair, outcat, gcat):
    """g_warped of warp_diff_norm_cat's backward (B x C x H x W) with the fused kernels' arithmetic."""
    C = pair.shape[1] // 2
    gn, nrm = gcat[:, 3 * C + 2:3 * C + 3], outcat[:, 3 * C + 2:3 * C + 3]
    diff = (pair[:, :C] - outcat[:, 2 * C:3 * C]).astype(np.float32)
    return (gcat[:, 2 * C:3 * C] - chnorm_grad(gn, diff, nrm)).astype(np.float32)


def warp_diff_norm_cat_grad_second(pair, flow, outcat, gcat):
    """grad_pair[:, C:] of the deterministic warp_diff_norm_cat backward: the concat gradient's slice, then the fixed-point scatter."""
    pair, outcat, gcat = (np.asarray(a, dtype=np.float32) for a in (pair, outcat, gcat))
    B, C2, H, W = pair.shape
    C = C2 // 2
    return resample_bwd_det((B, C, H, W), flow, warped_grad(pair, outcat, gcat), 1, grad_init=gcat[:, C:2 * C])


def exact_and_bound(img_shape, flow, gout, k=1):
    """float64 sum of every plane's fp32 contributions and the documented bound of |deterministic - exact| per cell: the quantisation
    (count * 2^(E+K-63)), the int64 -> double step (2^-53 relative) and the final fp32 rounding (half an ulp, subnormals included)."""
    B, C, Hi, Wi = img_shape
    _, _, H, W = gout.shape
    K = det_K(k, H, W)
    exact = np.zeros((B, C, Hi * Wi))
    bound = np.zeros((B, C, Hi * Wi))
    for b in range(B):
        geom = scatter_geometry(np.asarray(flow[b], np.float32), Hi, Wi, k)
        for c in range(C):
            g = np.asarray(gout[b, c], np.float32)
            v, cells = contributions(geom, g)
            exact[b, c] = np.bincount(cells, weights=v.astype(np.float64), minlength=Hi * Wi)
            kind, s = plane_scale(g, K)
            if kind != "finite":
                continue
            E = 62 - K - s
            count = np.bincount(cells, minlength=Hi * Wi).astype(np.float64)
            a = np.abs(exact[b, c])
            bound[b, c] = count * 2.0 ** (E + K - 63) + a * 2.0 ** -52 + np.maximum(a * 2.0 ** -24, 2.0 ** -150)
    return exact.reshape(B, C, Hi, Wi), bound.reshape(B, C, Hi, Wi)


# ---- the flows of the tests (shared by the host mutation check and the GPU tests)
def bench_flow(B, H, W, seed=0):
    """bench.py's flow: standard normal x 4 px."""
    return (np.random.default_rng(seed).standard_normal((B, 2, H, W)) * 4.0).astype(np.float32)


def translated_flow(B, H, W, seed=0, dx=25.0, dy=-18.0):
    """a translation of (dx, dy) px plus a little noise: the tiles' windows must follow the flow, the borders pile corners."""
    f = (np.random.default_rng(seed).standard_normal((B, 2, H, W)) * 0.5).astype(np.float32)
    f[:, 0] += np.float32(dx)
    f[:, 1] += np.float32(dy)
    return f


def sink_flow(B, H, W, seed=0, strength=0.7):
    """a converging flow: every pixel moves 70 % of the way towards the image centre, so many cells collect many contributions and
    most pixels of a tile land outside its window (the far-pixel path)."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f = np.empty((B, 2, H, W), np.float32)
    f[:, 0] = strength * ((W - 1) / 2.0 - xs)
    f[:, 1] = strength * ((H - 1) / 2.0 - ys)
    f += (np.random.default_rng(seed).standard_normal((B, 2, H, W)) * 0.3).astype(np.float32)
    return f
