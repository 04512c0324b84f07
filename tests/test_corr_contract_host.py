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
import test_bwd_u_range_host as S           # the schedule helpers
import test_gpu_corr_task_handover as T     # the shapes of the GPU cases (the modules import no GPU code)
import test_gpu_f32_contract as G
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


# ------------------------------------------------------------------ the multi-task cases of the GPU tests have power
# Conditions on the inputs and the schedule alone (no kernel): tests/test_gpu_f32_contract.py BWD_MULTI and
# tests/test_gpu_corr_task_handover.py mean something only if their workgroups do run several tasks and the tasks that follow
# each other differ by what a wrong hand-over would carry over.
NU = 6
HANDOVERS = {(11, 192, 14, 56): (264, 8), (3, 256, 48, 64): (288, 32), (22, 64, 48, 8): (528, 272), (1, 704, 48, 8): (264, 8)}


def _fwd_ntasks(B, H, W):
    """Tasks of a forward launch.  W <= 64 (f16x2_common.h build_task_table): 2 NRG NU per item, real and zero-only.  W > 64
    (correlation_f16x2_wide.hip build_pair_table): per parity and B row block b the row groups max(0, b - 5) .. min(b, NRG - 1)
    in pairs, times the ceil(W / 32) windows."""
    NRG = (H // 2 + 3) // 4
    if W <= 64:
        return B * 2 * NRG * NU
    k = S.src("correlation_f16x2_wide.hip")
    assert "constexpr int AW = 4;" in k and "constexpr int WPX = 8 * AW;" in k and "a.NXQ = (W + hw::WPX - 1) / hw::WPX;" in k
    pairs = sum((min(b, NRG - 1) - max(0, b - (NU - 1)) + 2) // 2 for b in range(NRG - 1 + NU))
    return B * 2 * pairs * -(-W // 32)


def _multi_case(shape):
    """(in1, in2, gradOutput) whose consecutive tasks differ: family 6 x 'items'; inside one item, the row ramp x 'items'."""
    return G.multi_inputs(shape, 6 if shape[0] > 1 else 5, "items")


def test_multi_task_shapes_exceed_the_grid():
    assert set(G.BWD_MULTI) == set(HANDOVERS)
    for shape, (ntasks, n_pairs) in HANDOVERS.items():
        B, C, H, W = shape
        pairs = S.handovers(*shape)
        assert S.bwd_ntasks(B, C, H) == ntasks > S.MAX_GRID and len(pairs) == S.MAX_GRID
        assert sum(len(p) for p in pairs) == n_pairs == ntasks - S.MAX_GRID
    assert max(len(p) for p in S.handovers(22, 64, 48, 8)) == 2 and min(len(p) for p in S.handovers(22, 64, 48, 8)) == 1
    # what each shape is in the table for
    assert all(n0 == 0 and n1 == 2 for w in S.handovers(3, 256, 48, 64) for (_, _, _, _, n0), (_, _, _, _, n1) in w)
    assert all(t0[4] == t1[4] == 0 and (t0[1], t1[1]) == (0, 5) and t0[2] != t1[2] and t0[3] != t1[3] and t0[0] != t1[0]
               for w in S.handovers(1, 704, 48, 8) for t0, t1 in w)
    assert all(t0[0] != t1[0] and t0[4] != t1[4] for w in S.handovers(11, 192, 14, 56) for t0, t1 in w)
    odd = lambda rg: (S.u_range(rg, 24)[1] - S.u_range(rg, 24)[0]) % 2 == 0
    kinds = {(odd(t0[1]), odd(t1[1])) for w in S.handovers(22, 64, 48, 8) for t0, t1 in w}
    assert {(False, True), (True, False), (False, False)} <= kinds                  # odd and even step counts follow each other
    # the schedule-independence cases
    for shape, _ in T.NARROW_BWD:
        assert S.bwd_ntasks(*shape[:3]) > S.MAX_GRID
    for shape in T.NARROW_FWD + [T.WIDE, T.LOWP]:
        assert _fwd_ntasks(shape[0], *shape[2:]) > S.MAX_GRID, shape
        assert _fwd_ntasks(1, *shape[2:]) <= S.MAX_GRID, shape                         # an item alone: one task per workgroup
    assert [_fwd_ntasks(s[0], *s[2:]) for s in T.NARROW_FWD + [T.WIDE, T.LOWP]] == [648, 288, 336, 336]
    B, C, H, W = T.WIDE
    nxw = -(-W // S.wpx_bwd_wide())
    assert nxw == 2 and S.bwd_ntasks(B, C, H, nxw) == 288 and S.bwd_ntasks(1, C, H, nxw) <= S.MAX_GRID
    assert sum(len(p) for p in S.handovers_wide(*T.WIDE)) == 32
    assert {(t0[4], t1[4]) for w in S.handovers_wide(*T.WIDE) for t0, t1 in w} == {(0, 1)}
    B, C, H, W = T.LOWP
    assert S.bwd_ntasks(B, C, H) == 448 and S.bwd_ntasks(1, C, H) <= S.MAX_GRID
    assert sum(len(p) for p in S.handovers(*T.LOWP, flip_outer=True)) == 448 - 256


def test_single_task_shapes_have_no_handover():
    """Why BWD_MULTI exists: on BWD_NARROW (4, 108 and 120 tasks) no workgroup of corr_bwd_f16x2 runs a second task."""
    for shape in G.BWD_NARROW:
        assert S.bwd_ntasks(*shape[:3]) <= S.MAX_GRID
        assert all(p == [] for p in S.handovers(*shape)), shape
    assert [S.bwd_ntasks(*s[:3]) for s in G.BWD_NARROW] == [4, 108, 120]


@pytest.mark.parametrize("shape", G.BWD_MULTI, ids=lambda s: "x".join(map(str, s)))
def test_handovers_change_the_magnitudes(shape):
    """At least half of a shape's hand-overs change the task's G magnitude (m_bwd_g at the task's rows) by 2^16 or more, and at
    least half change the X magnitude (m_bwd_x at the task's rows; here: of every channel of the task -- a channel keeps its
    place in scl_sx from task to task): an exponent or sample left over from the previous task is far outside the bound."""
    a, b, go = _multi_case(shape)
    B, C, H, W = shape
    mg = R.m_bwd_g(go, H, W)
    mx = (R.m_bwd_x(b), R.m_bwd_x(a))                       # X of a grad_in1 task is in2, of a grad_in2 task in1
    pairs = [p for w in S.handovers(*shape) for p in w]
    far = lambda u, v: bool((torch.maximum(u / v, v / u) >= 2.0 ** 16).all())
    g_of = lambda t: mg[t[4], 0, 8 * t[1], 0]
    x_of = lambda t: mx[t[2]][t[4], 64 * t[0]:64 * t[0] + 64, 8 * t[1], 0]
    ng = sum(far(g_of(t0), g_of(t1)) for t0, t1 in pairs)
    nx = sum(far(x_of(t0), x_of(t1)) for t0, t1 in pairs)
    print(f"{shape}: {len(pairs)} hand-overs, G magnitude changes at {ng}, X magnitude (every channel) at {nx}")
    assert 2 * ng >= len(pairs) and 2 * nx >= len(pairs)


@pytest.mark.parametrize("shape", G.BWD_MULTI, ids=lambda s: "x".join(map(str, s)))
def test_a_dropped_task_is_caught(shape):
    """An answer that leaves a task out (zeros, or whatever was there) is outside the bracket: |ref| > delta on at least 99 % of
    the gradient elements of every item a hand-over reaches (the items of the second and third tasks; the other items cost
    the same float64 passes again and show nothing else)."""
    a, b, go = _multi_case(shape)
    reached = sorted({t1[4] for w in S.handovers(*shape) for _, t1 in w})
    if shape == (22, 64, 48, 8):
        assert reached == list(range(10, 22))
    for n in reached:
        (r1, d1), (r2, d2), _ = R.bwd_deltas(a[n:n + 1], b[n:n + 1], go[n:n + 1], CORR)
        f1, f2 = float((r1.abs() > d1).double().mean()), float((r2.abs() > d2).double().mean())
        print(f"{shape} item {n}: |ref| > delta on {f1:.4f} (grad_input1), {f2:.4f} (grad_input2) of the elements")
        assert f1 >= 0.99 and f2 >= 0.99


def test_schedule_model_is_in_the_sources():
    """handovers() / handovers_wide() restate each kernel's get_task and the launchers' grid."""
    for name in S.BWD_FILES:
        k = S.src(name)
        assert "k.cg = t % p.NCGR; t /= p.NCGR;" in k and "k.rg = t % p.NRG; t /= p.NRG;" in k and "k.py = t & 1; t >>= 1;" in k, name
        assert "const unsigned grid = ntasks < 256 ? (unsigned)ntasks : 256u;" in k, name
        assert "xcd_remap(blockIdx.x, gridDim.x); t < ntasks; t += gridDim.x" in k, name
    k = S.src("correlation_f16x2_bwd.hip")
    order = ["k.cg = t % p.NCGR; t /= p.NCGR;", "k.rg = t % p.NRG; t /= p.NRG;", "#else\n        k.flip = p.nflip == 2 ? t % 2 : p.flip0;",
             "if (p.nflip == 2) t >>= 1;", "k.py = t & 1; t >>= 1;\n        k.n = t;"]
    at = [k.index(s) for s in order]
    assert at == sorted(at)
    assert "const long ntasks = 2L * B * 2 * a.NRG * a.NCGR;" in k and "a.nflip = 2; a.flip0 = 0;" in k
    for name in S.BWD_FILES[1:]:
        k = S.src(name)
        assert "k.py = t & 1; t >>= 1;\n        k.n = t % p.B;\n        k.flip = t / p.B;" in k, name
    k = S.src("correlation_f16x2_bwd_wide.hip")
    at = [k.index(s) for s in ("k.cg = t % p.NCGR; t /= p.NCGR;", "k.xw = t % p.NXW; t /= p.NXW;", "k.rg = t % p.NRG; t /= p.NRG;")]
    assert at == sorted(at)
    assert "a.NXW = (W + hbw::WPX - 1) / hbw::WPX;" in k and "const long ntasks = 2L * B * 2 * a.NRG * a.NXW * a.NCGR;" in k
    assert S.wpx_bwd_wide() == 64
    assert "const long ntasks = 2L * B * 2 * a.NRG * a.NCGR;" in S.src("correlation_f16_bwd.hip")
