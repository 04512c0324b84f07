"""float64 numpy reference of Correlation1d (include/flownet2_hip_ext.h) -- TEST INFRASTRUCTURE ONLY, not a test file.

    out[b,o,y,x]      = (1/C) sum_c in1[b,c,y1,x1] * in2[b,c,y1,x1 + t s2],     y1 = y s1, x1 = x s1 + md - pad, t = t_min + o
    grad_in1[b,c,y,x] = (1/C) sum_t gO[b,o,y,x+pad-md]      * in2[b,c,y,x+t s2]                        (s1 = 1)
    grad_in2[b,c,y,x] = (1/C) sum_t gO[b,o,y,x-t s2+pad-md] * in1[b,c,y,x-t s2]

A term whose operand column or output column lies outside is absent.  Every function returns, per element, the exact value (of
the operands' finite parts), the sum of |products| / C over the element's terms (what the error bounds scale with) and a mask
of elements that have a term whose product is not finite (an operand of it is inf or nan): there the kernels' results are not
finite, everywhere else they are."""
import numpy as np

U23 = 2.0 ** -23


def displacements(md, s2, sd):
    dr = md // s2
    return list(range(-dr if sd != 1 else 0, (dr if sd != -1 else 0) + 1))


def out_shape(H, W, pad, md, s1, s2, sd=0):
    """(nOut, oH, oW) of fn2x_correlation1d_output_shape."""
    return len(displacements(md, s2, sd)), -(-H // s1), -(-(W + 2 * pad - 2 * md) // s1)


def _split(x):
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    return np.where(fin, x, 0.0), (~fin).astype(np.float64)


def forward(a, b, pad, md, s1, s2, sd=0):
    """(exact, abs_sum, nonfinite), each (B, nOut, oH, oW)."""
    a, na = _split(a)
    b, nb = _split(b)
    B, C, H, W = a.shape
    nOut, oH, oW = out_shape(H, W, pad, md, s1, s2, sd)
    ref = np.zeros((B, nOut, oH, oW))
    absr = np.zeros_like(ref)
    bad = np.zeros_like(ref)
    ys = np.arange(oH) * s1
    x1 = np.arange(oW) * s1 + md - pad
    for o, t in enumerate(displacements(md, s2, sd)):
        x2 = x1 + t * s2
        ok = (x1 >= 0) & (x1 < W) & (x2 >= 0) & (x2 < W)
        c1, c2 = np.clip(x1, 0, W - 1), np.clip(x2, 0, W - 1)
        pa, pb = a[:, :, ys][:, :, :, c1], b[:, :, ys][:, :, :, c2]
        ref[:, o] = np.where(ok, (pa * pb).sum(1), 0.0)
        absr[:, o] = np.where(ok, np.abs(pa * pb).sum(1), 0.0)
        bad[:, o] = np.where(ok, (na[:, :, ys][:, :, :, c1] + nb[:, :, ys][:, :, :, c2]).sum(1), 0.0)
    return ref / C, absr / C, bad > 0


def backward(a, b, go, pad, md, s1, s2, sd=0):
    """((exact1, abs_sum1, nonfinite1), (exact2, abs_sum2, nonfinite2)) of grad_in1 / grad_in2, each (B, C, H, W); stride1 = 1."""
    assert s1 == 1, "the backward is defined for stride1 = 1 only"
    a, na = _split(a)
    b, nb = _split(b)
    go, ng = _split(go)
    B, C, H, W = a.shape
    nOut, oH, oW = out_shape(H, W, pad, md, s1, s2, sd)
    assert go.shape == (B, nOut, oH, oW), (go.shape, (B, nOut, oH, oW))
    res = [[np.zeros((B, C, H, W)) for _ in range(3)] for _ in range(2)]
    x = np.arange(W)
    for o, t in enumerate(displacements(md, s2, sd)):
        # grad_in1: gO at column x + pad - md, in2 at column x + t s2;  grad_in2: both at the in1 pixel x - t s2
        for which, (inp, ninp, xo) in enumerate(((b, nb, x + t * s2), (a, na, x - t * s2))):
            ox = (x if which == 0 else xo) + pad - md
            ok = (xo >= 0) & (xo < W) & (ox >= 0) & (ox < oW)
            g = go[:, o][:, None, :, np.clip(ox, 0, oW - 1)]
            v = inp[:, :, :, np.clip(xo, 0, W - 1)]
            nf = ng[:, o][:, None, :, np.clip(ox, 0, oW - 1)] + ninp[:, :, :, np.clip(xo, 0, W - 1)]
            res[which][0] += np.where(ok, g * v, 0.0)
            res[which][1] += np.where(ok, np.abs(g * v), 0.0)
            res[which][2] += np.where(ok, nf, 0.0)
    return tuple((r[0] / C, r[1] / C, r[2] > 0) for r in res)


def delta_fwd_f32(ref, absr, C):
    """Forward bound of the header for fp32 (and for double tensors, whose forward accumulates in float)."""
    return (C // 4 + C % 4 + 4) * U23 * absr + U23 * np.abs(ref)


def delta_bwd_f32(ref, absr, nOut):
    return (nOut + 1) * U23 * absr + U23 * np.abs(ref)
