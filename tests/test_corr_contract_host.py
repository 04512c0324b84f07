"""The bounds of tests/corr_contract_ref.py on the CPU, no GPU: a numpy model of the narrow f16x2 forward (the split of
tests/test_split_model.py, one scale per operand and task from the kernel's own sample positions, fp32 sums of the three partial
products, the epilogue of correlation_f16x2.hip) meets them on every input family; four plausible wrong kernels -- the same
model with one change each -- leave them.  For each mutation the test prints whether the suite's older global checks (maximum
absolute error 2e-6; worst error relative to the largest output within 3x a plain fp32 sum's) would have accepted it."""
import numpy as np
import pytest
import torch

import corr_contract_ref as R
import lowp_ref as L
from test_split_model import split

CORR = L.CORR
DR = 10


def _scale_exp(vals):
    """f16x2_split.h scale_exp on a sample: mean biased exponent of the values with a non-zero exponent field, k = T_GEO + 127 -
    round(mean), clamped to -126 .. 127; no such value: k = 0."""
    e = ((np.asarray(vals, np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    e = e[e != 0]
    if e.size == 0:
        return 0
    return int(np.clip(-1 + 127 - int(np.float32(e.sum()) / np.float32(e.size) + np.float32(0.5)), -126, 127))


def _sample(x, n, py, il0, C, H, W):
    """The 256 values sample_issue (correlation_f16x2.hip) reads for lattice rows il0 .. il0 + 3 of parity py; rows outside the
    image read zeros."""
    HL = H // 2
    out = []
    for ln in range(64):
        c, r = (ln * C) >> 6, ln & 3
        xs = 4 * (((((5 * ln) >> 2) & 15) * (W >> 2)) >> 4)
        il = il0 + r
        out.extend(x[n, c, 2 * il + py, xs:xs + 4] if 0 <= il < HL else np.zeros(4, np.float32))
    return np.array(out, np.float32)


def model_fwd(a, b, mutation=None):
    """Narrow f16x2 forward (pad = md = 20, s2 = 2) in numpy: per output ka of the A task (n, py, rg), kb of the B row block;
    products ah bh + ah bl + al bh summed in fp32 over the channels; non-finite sums recomputed by an fp32 fma-free chain (the
    recompute's bound is the larger chain bound); ldexp by -(ka + kb), then / C for a C that is no power of two.
    mutation: 'other_item' (a) scales from the next batch item's samples; 'flush_l' (b) l flushed where it is an f16 subnormal;
    'drop_albh' (c) the al bh product dropped; 'ftz_epilogue' (d) the scale removed before the 1/C with fp32 subnormals
    flushed to zero."""
    B, C, H, W = a.shape
    HL = H // 2
    out = np.zeros((B, 441, H, W), np.float32)
    f = np.float32
    for n in range(B):
        ns = (n + 1) % B if mutation == "other_item" else n
        for py in range(2):
            for IL in range(HL):
                y = 2 * IL + py
                ka = _scale_exp(_sample(a, ns, py, 4 * (IL // 4), C, H, W))
                _, ah, al = split(a[n, :, y, :], ka)
                for tj in range(21):
                    ILb = IL + tj - DR
                    if not 0 <= ILb < HL:
                        continue
                    q0 = 4 * ((ILb - 2) // 4) + 2
                    kb = _scale_exp(_sample(b, ns, py, q0, C, H, W))
                    _, bh, bl = split(b[n, :, 2 * ILb + py, :], kb)
                    pad = lambda t: np.pad(t.astype(f), ((0, 0), (DR * 2, DR * 2)))
                    cols = np.arange(W)[None, :] + 2 * np.arange(21)[:, None]          # (ti, x) -> padded B column
                    B_h, B_l, B_x = pad(bh)[:, cols], pad(bl)[:, cols], pad(b[n, :, 2 * ILb + py, :])[:, cols]   # (C, ti, x)
                    A_h, A_l = ah.astype(f), al.astype(f)
                    if mutation == "flush_l":
                        A_l = np.where(np.abs(A_l) < 2.0 ** -14, f(0), A_l)
                        B_l = np.where(np.abs(B_l) < 2.0 ** -14, f(0), B_l)
                    acc = np.zeros((21, W), f)
                    with np.errstate(all="ignore"):
                        for c in range(C):
                            acc = acc + A_h[c] * B_h[c]
                            acc = acc + A_h[c] * B_l[c]
                            if mutation != "drop_albh":
                                acc = acc + A_l[c] * B_h[c]
                        v = np.ldexp(acc.astype(np.float64), -(ka + kb))
                        bad = ~np.isfinite(acc)
                        if bad.any():   # the fp32 recompute
                            ex = np.zeros((21, W), f)
                            for c in range(C):
                                ex = ex + a[n, c, y].astype(f) * B_x[c]
                            v = np.where(bad, ex.astype(np.float64), v)
                    if mutation == "ftz_epilogue":
                        v = np.where(np.abs(v) < 2.0 ** -126, 0.0, v)
                    v32 = v.astype(f)                                          # ldexp into fp32 (one rounding if subnormal)
                    valid = (np.arange(W)[None, :] + 2 * (np.arange(21)[:, None] - DR) >= 0) & (cols - 2 * DR < W)
                    out[n, tj * 21:tj * 21 + 21, y, :] = np.where(valid, v32 / f(C), f(0))
    return out


def fp32_plain(a, b):
    """The plain fp32 sum the older global checks compared against (a product, then a sum, per channel)."""
    B, C, H, W = a.shape
    out = np.zeros((B, 441, H, W), np.float32)
    for tj in range(21):
        for ti in range(21):
            dy, dx = 2 * (tj - DR), 2 * (ti - DR)
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            acc = np.zeros((B, y1 - y0, x1 - x0), np.float32)
            with np.errstate(all="ignore"):
                for c in range(C):
                    acc = acc + a[:, c, y0:y1, x0:x1] * b[:, c, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            out[:, tj * 21 + ti, y0:y1, x0:x1] = acc / np.float32(C)
    return out


def _bracket_ok(out, a, b):
    """(all inside, worst err/delta) of the f16x2 forward bound on the model's output."""
    at, bt = torch.from_numpy(a), torch.from_numpy(b)
    nonfin = R.fwd_nonfinite(at, bt, CORR)
    ref, absr, s1, s2, s3 = R.fwd_sums(at, bt, CORR, wide=False)
    delta = R.delta_f16x2_fwd(ref, absr, s1, s2, s3, a.shape[1])
    ia = (~(at.abs() < 65520)).double().amax(1, keepdim=True).expand_as(at).contiguous()
    ib = (~(bt.abs() < 65520)).double().amax(1, keepdim=True).expand_as(bt).contiguous()
    one = torch.ones_like(ia)
    touched = (L.corr_fwd64(ia, one, *CORR) + L.corr_fwd64(one, ib, *CORR)) > 0
    delta = torch.where(touched, R.delta_fma_chain(ref, absr, a.shape[1]), delta)
    got = torch.from_numpy(out)
    fin = ~nonfin
    if not torch.equal(torch.isfinite(got), fin):
        return False, float("inf")
    lo, hi = L.bracket(ref[fin], delta[fin], torch.float32)
    inside = not bool(L.outside(got[fin], lo, hi).any())
    ratio = float(((got[fin].double() - ref[fin]).abs() / delta[fin].clamp(min=1e-300)).max())
    return inside, ratio


def _old_checks(out, a, b):
    """The suite's global assertions, each on its own, as (verdict, the inputs it is asserted on): max |out - ref| <= 2e-6 on
    unit-normal inputs (the oracle and fuzz tests); the worst error relative to the largest output within 3x that of a plain
    fp32 sum (+ 2^-24) at any magnitude (the magnitude sweeps); max |out - ref| <= 1e-9 on 1e-3 data whose samples read only
    zeros (test_correlation_f16x2_scale_sample_misses)."""
    ref = L.corr_fwd64(torch.from_numpy(a), torch.from_numpy(b), *CORR).numpy()
    fin = np.isfinite(ref) & np.isfinite(out)
    with np.errstate(invalid="ignore"):
        err = np.abs(out.astype(np.float64) - ref)[fin]
        e32 = np.abs(fp32_plain(a, b).astype(np.float64) - ref)[fin]
    big = np.abs(ref[fin]).max()
    return {"absolute 2e-6 (unit normal)": bool(err.max() <= 2e-6),
            "relative (magnitude sweeps)": bool(err.max() / big <= 3 * e32.max() / big + 2.0 ** -24),
            "absolute 1e-9 (sample misses)": bool(err.max() <= 1e-9)}


SHAPE = (3, 64, 8, 16)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_model_meets_the_bound(family):
    a, b = (t.numpy() for t in R.family_inputs(family, SHAPE, seed=family))
    inside, ratio = _bracket_ok(model_fwd(a, b), a, b)
    print(f"family {family}: correct model, worst err/delta {ratio:.3g}")
    assert inside, (family, ratio)


# (mutation, family, shape, the older check that applies to that family's inputs)
MUTATIONS = [("other_item", 6, (2, 64, 8, 16), "relative (magnitude sweeps)"),
             ("flush_l", 10, (1, 64, 8, 16), "absolute 1e-9 (sample misses)"),
             ("drop_albh", 1, (1, 64, 8, 16), "absolute 2e-6 (unit normal)"),
             ("ftz_epilogue", 8, (2, 192, 8, 16), "relative (magnitude sweeps)")]


@pytest.mark.parametrize("mutation,family,shape,old_check", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_bound_rejects_wrong_kernels(mutation, family, shape, old_check):
    """(a) scales from another batch item's sample, on items at 2^+30 / 2^-30 (the large item's operands overflow the f16 under
    the small item's scale and are recomputed exactly; the small item's vanish); (b) l flushed where it is an f16 subnormal, on 1e-3
    data whose samples read only zeros (unscaled: every l is an f16 subnormal); (c) al bh dropped; (d) the scale removed with subnormals
    flushed before the 1/C (non-power-of-two C), on outputs near 2^-132.  The older verdict printed and asserted is that of the
    older check asserted on inputs like these; the others are printed for information."""
    a, b = (t.numpy() for t in R.family_inputs(family, shape, seed=3))
    good, _ = _bracket_ok(model_fwd(a, b), a, b)
    assert good
    out = model_fwd(a, b, mutation)
    old = _old_checks(out, a, b)
    inside, ratio = _bracket_ok(out, a, b)
    verdict = lambda ok: "ACCEPT" if ok else "reject"
    others = ", ".join(f"{k} {verdict(v)}" for k, v in old.items() if k != old_check)
    print(f"mutation {mutation} (family {family}): older check {old_check}: {verdict(old[old_check])} [{others}]; "
          f"per-element bound {'accept' if inside else 'REJECT'} (worst err/delta {ratio:.3g})")
    assert not inside
    if mutation in ("other_item", "flush_l"):
        assert old[old_check], "the older check was expected to accept this mutation"
