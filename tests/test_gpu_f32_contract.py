"""The float32 and float64 correlation kernels against their documented error bounds, element by element
(include/flownet2_hip.h at FN2_CORR_MFMA_F16X2, _BF16X3, _MFMA_F32, _DIRECT and the fp64 kernel; the bounds and their
derivations: tests/corr_contract_ref.py).  Every output element must lie in the fp32 bracket of its float64 reference widened by
its own bound; operands carry full 24-bit mantissas (an f16 split then has a non-zero low term), batch items and column windows
carry different magnitudes (a scale taken from the wrong task's sample leaves the bracket), and the bound's floor scales with
the task's typical magnitude m, bounded from the sample code.

Every case also checks that no output was left unwritten (outputs prefilled with NaN), names the kernel that ran by a
bit-identical pair (AUTO == the explicit selector, or the explicit selector declines with FN2_EUNSUPPORTED and AUTO equals the
kernel it falls back to), and prints the worst err / delta."""
import pytest
import torch

import corr_contract_ref as R
import lowp_ref as L

pytestmark = pytest.mark.gpu

CORR = L.CORR
SLOPE = 0.1
EUNSUPPORTED = "code -4"
F32 = torch.float32


def _nan(shape, dev, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _check(got, ref, delta, what, dtype=F32, post=None, nonfinite=None):
    """Every element in its bracket; non-finite exactly where expected (`nonfinite`: corr_contract_ref.fwd_nonfinite; else where
    the float64 reference is); returns and prints the worst err/delta."""
    fin = torch.isfinite(ref) if nonfinite is None else ~nonfinite
    assert torch.equal(torch.isfinite(got), fin), f"{what}: non-finite outputs differ from the reference's"
    ref, delta, g = ref[fin], delta[fin], got[fin]
    if dtype == F32:
        lo, hi = L.bracket(ref, delta, F32, post=post) if post is None else _bracket32(ref, delta, post)
    else:
        lo, hi = ref - delta, ref + delta
    L.check_bracket(g, lo, hi, what)
    target = ref if post is None else post(ref)
    ratio = float(((g.double() - target).abs() / delta.clamp(min=1e-300)).max()) if g.numel() else 0.0
    print(f"  {what}: worst err/delta {ratio:.3g}")
    return ratio


def _bracket32(ref, delta, post):
    lo, hi = L._f32_down(ref - delta), L._f32_up(ref + delta)
    return post(lo), post(hi)


def _leaky(x):
    s = torch.tensor(SLOPE, dtype=x.dtype, device=x.device)
    return torch.where(x > 0, x, x * s)


def _run_fwd(ad, bd, params, algo):
    import fn2_capi
    B, C, H, W = ad.shape
    out = _nan((B,) + L.out_shape(H, W, *params), ad.device, ad.dtype)
    fn2_capi.correlation_forward(ad, bd, *params, algo=algo, out=out)
    assert not torch.isnan(out).any() or bool(torch.isnan(ad).any() | torch.isnan(bd).any()), "unwritten output elements"
    return out


def _run_bwd(ad, bd, gd, params, algo):
    """Both gradients of the selected kernel, written into NaN-prefilled outputs; every element must be written."""
    import fn2_capi
    g1, g2 = _nan(ad.shape, ad.device, ad.dtype), _nan(bd.shape, bd.device, bd.dtype)
    fn2_capi.correlation_backward(ad, bd, gd, *params, algo=algo, out=(g1, g2))
    assert not (torch.isnan(g1).any() or torch.isnan(g2).any()), "unwritten gradient elements"
    return g1, g2


def _touched_fwd(ad, bd, params, thresh=65520.0):
    """Outputs whose terms include an operand the f16 split cannot hold (|x| >= 65520 with m <= 1/2 here)."""
    ia = (~(ad.abs() < thresh)).double().amax(1, keepdim=True).expand_as(ad).contiguous()
    ib = (~(bd.abs() < thresh)).double().amax(1, keepdim=True).expand_as(bd).contiguous()
    one = torch.ones_like(ia)
    return (L.corr_fwd64(ia, one, *params) + L.corr_fwd64(one, ib, *params)) > 0


# ------------------------------------------------------------------ f16x2 forward
FWD_NARROW = [(1, 64, 2, 8), (9, 192, 6, 56), (1, 256, 46, 64), (9, 320, 48, 8), (1, 64, 48, 64)]
FWD_WIDE = [(1, 64, 6, 72), (2, 192, 46, 128), (1, 320, 2, 136), (1, 64, 48, 200), (8, 256, 56, 128)]


def _f16x2_fwd_case(dev, shape, fam, fused=True):
    import fn2_capi
    a, b = R.family_inputs(fam, shape, seed=sum(shape))
    ad, bd = a.to(dev), b.to(dev)
    B, C, H, W = shape
    out = _run_fwd(ad, bd, CORR, fn2_capi.FN2_CORR_AUTO)
    sel = _run_fwd(ad, bd, CORR, fn2_capi.FN2_CORR_MFMA_F16X2)
    assert torch.equal(sel.view(torch.int32), out.view(torch.int32)), f"{shape} family {fam}: AUTO is not the f16x2 kernel"
    nonfin = R.fwd_nonfinite(ad, bd, CORR)
    ref, absr, s_mb_a, s_ma_b, s_mm = R.fwd_sums(ad, bd, CORR, wide=W > 64)
    delta = R.delta_f16x2_fwd(ref, absr, s_mb_a, s_ma_b, s_mm, C)
    if fam == 9:
        # the outputs an out-of-range operand touches: the fp32 fma chain's bound
        t = _touched_fwd(ad, bd, CORR)
        assert bool(t.any()) and bool(nonfin.any())
        delta = torch.where(t, R.delta_fma_chain(ref, absr, C), delta)
        # inf / nan next to the padding: non-finite exactly where the general kernel's outputs are (absent terms)
        direct = _run_fwd(ad, bd, CORR, fn2_capi.FN2_CORR_DIRECT)
        assert torch.equal(torch.isfinite(direct), ~nonfin), f"{shape}: the general kernel's non-finite outputs"
    worst = _check(out, ref, delta, f"f16x2 fwd {shape} family {fam}", nonfinite=nonfin)
    if fused:
        nOut = out.shape[1]
        g = torch.Generator(device=dev).manual_seed(sum(shape))
        buf = torch.randn((B, 8 + nOut + 3) + out.shape[2:], generator=g, device=dev)
        buf[:, 8:8 + nOut] = float("nan")
        before = buf.clone()
        fn2_capi.correlation_forward_fused(ad, bd, buf, 8, SLOPE, *CORR)
        assert torch.equal(buf[:, :8].view(torch.int32), before[:, :8].view(torch.int32))
        assert torch.equal(buf[:, 8 + nOut:].view(torch.int32), before[:, 8 + nOut:].view(torch.int32))
        worst = max(worst, _check(buf[:, 8:8 + nOut], ref, delta, f"f16x2 fwd fused {shape} family {fam}", post=_leaky,
                                  nonfinite=nonfin))
    return worst


@pytest.mark.parametrize("shape", FWD_NARROW + FWD_WIDE, ids=lambda s: "x".join(map(str, s)))
def test_f16x2_forward(dev, shape):
    """Every family, plain and fused (family 6 at B = 1 is one item at 2^30; family 8 at B = 1 is item 0 alone, at 2^-66)."""
    for fam in R.FAMILIES:
        _f16x2_fwd_case(dev, shape, fam)


# ------------------------------------------------------------------ f16x2 backward
BWD_NARROW = [(1, 64, 2, 8), (9, 192, 6, 56), (1, 320, 48, 64)]
BWD_WIDE = [(1, 64, 6, 72), (2, 192, 46, 128), (1, 320, 2, 136)]
GRADS = ("normal", "leaky", "window", "planes", "train")


def _bwd_case(dev, a, b, go, what):
    import fn2_capi
    ad, bd, gd = a.to(dev), b.to(dev), go.to(dev)
    g1, g2 = _nan(a.shape, dev), _nan(a.shape, dev)
    fn2_capi.correlation_backward(ad, bd, gd, *CORR, out=(g1, g2))
    s1, s2 = fn2_capi.correlation_backward(ad, bd, gd, *CORR, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
    assert torch.equal(s1.view(torch.int32), g1.view(torch.int32)) and torch.equal(s2.view(torch.int32), g2.view(torch.int32)), what
    nf1, nf2 = R.bwd_nonfinite(ad, bd, gd, CORR)
    if bool(nf1.any() | nf2.any()):   # the general kernel's non-finite gradients are the same
        e1, e2 = fn2_capi.correlation_backward(ad, bd, gd, *CORR, algo=fn2_capi.FN2_CORR_DIRECT)
        assert torch.equal(torch.isfinite(e1), ~nf1) and torch.equal(torch.isfinite(e2), ~nf2), what
    (r1, d1), (r2, d2), (ab1, ab2) = R.bwd_deltas(ad, bd, gd, CORR)
    w = _check(g1, r1, d1, what + " grad_input1", nonfinite=nf1)
    return max(w, _check(g2, r2, d2, what + " grad_input2", nonfinite=nf2))


@pytest.mark.parametrize("shape", BWD_NARROW + BWD_WIDE, ids=lambda s: "x".join(map(str, s)))
def test_f16x2_backward(dev, shape):
    B, C, H, W = shape
    nOut, oH, oW = L.out_shape(H, W, *CORR)
    for fam in R.FAMILIES:
        a, b = R.family_inputs(fam, shape, seed=sum(shape))
        go = R.grad_output("normal", (B, nOut, oH, oW), sum(shape) + fam)
        if fam == 8:   # gradOutput at the items' scale too: gradients near 2^-132 (fp32 subnormals) and 2^60
            go = go * torch.where(torch.arange(B) == 0, 2.0 ** -66, 2.0 ** 30).float().view(B, 1, 1, 1)
        _bwd_case(dev, a, b, go, f"f16x2 bwd {shape} family {fam}")
    a, b = R.family_inputs(1, shape, seed=sum(shape))
    for kind in GRADS[1:]:
        go = R.grad_output(kind, (B, nOut, oH, oW), sum(shape))
        _bwd_case(dev, a, b, go, f"f16x2 bwd {shape} family 1, gradOutput {kind}")


# Workgroups that run several tasks.  corr_bwd_f16x2 is persistent: min(ntasks, 256) workgroups, ntasks = 2 B 2 NRG (C / 64), and
# everything between two tasks of one workgroup -- the next task's operand sample and scale exponents (the other half of scl_sx,
# scl_k[1]), the prefetch of its first X chunks and G image, the hand-over of the register sets after an odd step count -- runs
# only past 256 tasks: BWD_NARROW above has 4, 108 and 120.  The smallest shapes that have each hand-over (counted by
# test_bwd_u_range_host.handovers; tests/test_corr_contract_host.py checks the counts and that the inputs tell the tasks apart):
BWD_MULTI = [
    (11, 192, 14, 56),   # 264 tasks, 8 hand-overs: the tail; ragged last row group (HL = 7), partial width, C no power of two,
                         # another channel group and item at the hand-over
    (3, 256, 48, 64),    # 288 tasks, 32: the benchmark's row geometry and full width, item 0 -> item 2
    (22, 64, 48, 8),     # 528 tasks, 272: two and three tasks per workgroup (the scl_sx half is reused), odd and even step counts
    (1, 704, 48, 8),     # 264 tasks, 8: inside one item -- row group 0 -> 5, gradient and parity flip, another channel group
]
# (family, gradOutput kind): in1 / in2 that differ per channel (2), row (5), item (6, 8), and gradOutput that differs per item
# or row band ("items"), so that consecutive tasks of a workgroup have other scale exponents
MULTI_INPUTS = [(2, "normal"), (5, "normal"), (6, "normal"), (8, "normal"), (6, "items"), (1, "items"), (1, "train")]


def multi_inputs(shape, fam, kind):
    """in1, in2, gradOutput (CPU float32) of a BWD_MULTI case; family 8 keeps test_f16x2_backward's item scaling of gradOutput."""
    B, C, H, W = shape
    nOut, oH, oW = L.out_shape(H, W, *CORR)
    a, b = R.family_inputs(fam, shape, seed=sum(shape))
    go = R.grad_output(kind, (B, nOut, oH, oW), sum(shape) + fam)
    if fam == 8:
        go = go * torch.where(torch.arange(B) == 0, 2.0 ** -66, 2.0 ** 30).float().view(B, 1, 1, 1)
    return a, b, go


@pytest.mark.parametrize("fam,kind", MULTI_INPUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", BWD_MULTI, ids=lambda s: "x".join(map(str, s)))
def test_f16x2_backward_multi_task_workgroups(dev, shape, fam, kind):
    """The per-element bound of test_f16x2_backward (bwd_deltas, every element: no family here is non-finite), AUTO == the
    explicit selector and fully written outputs, where a workgroup runs two or three tasks whose operands have other
    magnitudes."""
    a, b, go = multi_inputs(shape, fam, kind)
    assert bool(torch.isfinite(a).all() & torch.isfinite(b).all() & torch.isfinite(go).all())
    _bwd_case(dev, a, b, go, f"f16x2 bwd multi {shape} family {fam}, gradOutput {kind}")


@pytest.mark.parametrize("shape", [(2, 192, 46, 56), (1, 64, 48, 72), (22, 64, 48, 8)], ids=["narrow", "wide", "multi_task"])
def test_f16x2_backward_fused(dev, shape):
    """backward_fused against the float64 backward of the LeakyReLU-masked gradient, and bit-identical to the unfused backward
    (multi_task: 528 tasks, two and three per workgroup)."""
    import fn2_capi
    B, C, H, W = shape
    a, b = R.family_inputs(3, shape, seed=sum(shape))
    ad, bd = a.to(dev), b.to(dev)
    buf = torch.zeros((B, 8 + 441, H, W), device=dev)
    fn2_capi.correlation_forward_fused(ad, bd, buf, 8, SLOPE, *CORR)
    gbuf = R.grad_output("normal", tuple(buf.shape), sum(shape)).to(dev)
    masked = torch.ops.aten.leaky_relu_backward(gbuf[:, 8:].contiguous(), buf[:, 8:].contiguous(), SLOPE, True)
    f1, f2 = fn2_capi.correlation_backward_fused(ad, bd, buf, gbuf, 8, SLOPE, *CORR)
    u1, u2 = fn2_capi.correlation_backward(ad, bd, masked, *CORR, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
    assert torch.equal(f1, u1) and torch.equal(f2, u2)
    (r1, d1), (r2, d2), _ = R.bwd_deltas(ad, bd, masked, CORR)
    _check(f1, r1, d1, f"fused bwd {shape} grad_input1")
    _check(f2, r2, d2, f"fused bwd {shape} grad_input2")


# ------------------------------------------------------------------ launcher limits
@pytest.mark.parametrize("shape,accepted", [((1, 64, 512, 8), True), ((1, 64, 514, 8), False),
                                            ((6553, 64, 2, 8), True), ((6554, 64, 2, 8), False),
                                            ((2184, 64, 2, 72), True), ((2185, 64, 2, 72), False)],
                         ids=["H512", "H514", "Bnarrow_last", "Bnarrow_first_declined", "Bwide_last", "Bwide_first_declined"])
def test_f16x2_launcher_limits(dev, shape, accepted):
    """The last accepted / first declined shape of the forward launcher, each checked under the bound of the kernel that ran
    (declined: AUTO falls back to the bf16x3 kernel where W <= 64, else the fp32 MFMA kernel, bit-identical to its selector).  At H = 2 an item has 10 zero-only tasks
    (f16x2_common.h build_task_table; the wide kernel: 10 per window, 3 windows at W = 72): B x 10 (x 3) < 65536 is accepted.  Large batches: the items where the
    persistent workgroups' streams start and end are checked."""
    import fn2_capi
    g = torch.Generator().manual_seed(sum(shape))
    B, C, H, W = shape
    a = torch.randn(shape, generator=g).to(dev)
    b = torch.randn(shape, generator=g).to(dev)
    out = _run_fwd(a, b, CORR, fn2_capi.FN2_CORR_AUTO)
    if accepted:
        sel = _run_fwd(a, b, CORR, fn2_capi.FN2_CORR_MFMA_F16X2)
    else:
        with pytest.raises(RuntimeError, match=EUNSUPPORTED):
            fn2_capi.correlation_forward(a, b, *CORR, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
        # AUTO's next kernels in order: bf16x3 where its forward preconditions hold (W <= 64), else the fp32 MFMA kernel
        fallback = fn2_capi.FN2_CORR_MFMA_BF16X3 if _bf16x3_fwd_ok(C, W, 20) else fn2_capi.FN2_CORR_MFMA_F32
        sel = _run_fwd(a, b, CORR, fallback)
    assert torch.equal(sel.view(torch.int32), out.view(torch.int32))
    del sel
    items = sorted({i for i in (0, 1, B // 8, B // 8 + 1, B // 2, B - 2, B - 1) if 0 <= i < B})
    for i in items:
        ai, bi = a[i:i + 1], b[i:i + 1]
        if accepted:
            ref, absr, s1, s2, s3 = R.fwd_sums(ai, bi, CORR, wide=W > 64)
            delta = R.delta_f16x2_fwd(ref, absr, s1, s2, s3, C)
        else:
            ref = L.corr_fwd64(ai, bi, *CORR)
            absr = L.corr_fwd64(ai.abs(), bi.abs(), *CORR)
            delta = R.delta_bf16x3(ref, absr, C) if _bf16x3_fwd_ok(C, W, 20) else R.delta_fma_chain(ref, absr, C)
        _check(out[i:i + 1], ref, delta, f"{shape} item {i} ({'f16x2' if accepted else 'fallback'})")


# ------------------------------------------------------------------ bf16x3 and fp32 MFMA on their domains
MFMA_CASES = [(2, (2, 16, 10, 14)), (12, (1, 32, 14, 22)), (20, (2, 96, 10, 30)), (21, (1, 32, 12, 18)), (20, (1, 64, 8, 20))]


def _bf16x3_fwd_ok(C, W, md):
    return C % 32 == 0 and W <= 64 and (md // 2) % 2 == 0


def _maybe(run):
    """The explicit selector's result, or None where its launcher declines (FN2_EUNSUPPORTED, printed): that names the kernel."""
    try:
        return run()
    except RuntimeError as e:
        assert EUNSUPPORTED in str(e), e
        print("  declined (FN2_EUNSUPPORTED)")
        return None


@pytest.mark.parametrize("case", MFMA_CASES, ids=lambda c: f"md{c[0]}_C{c[1][1]}_W{c[1][3]}")
def test_fp32_mfma_kernels(dev, case):
    import fn2_capi
    md, shape = case
    params = (md, 1, md, 1, 2)
    B, C, H, W = shape
    nOut, oH, oW = L.out_shape(H, W, *params)
    for fam in (1, 2, 3, 4, 5, 7):
        a, b = R.family_inputs(fam, shape, seed=sum(shape))
        ad, bd = a.to(dev), b.to(dev)
        ref = L.corr_fwd64(ad, bd, *params)
        absr = L.corr_fwd64(ad.abs(), bd.abs(), *params)
        f32 = _run_fwd(ad, bd, params, fn2_capi.FN2_CORR_MFMA_F32)
        _check(f32, ref, R.delta_fma_chain(ref, absr, C), f"fp32 MFMA fwd md {md} {shape} family {fam}")
        x3 = _maybe(lambda: _run_fwd(ad, bd, params, fn2_capi.FN2_CORR_MFMA_BF16X3))
        if x3 is not None:
            _check(x3, ref, R.delta_bf16x3(ref, absr, C), f"bf16x3 fwd md {md} {shape} family {fam}")
        go = R.grad_output("normal", (B, nOut, oH, oW), sum(shape) + fam).to(dev)
        r1, r2 = L.corr_bwd64(ad, bd, go, *params)
        ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), go.abs(), *params)
        n = L.n_bwd(md, 2, 1)
        for algo, name, dl in ((fn2_capi.FN2_CORR_MFMA_F32, "fp32 MFMA", R.delta_fma_chain),
                               (fn2_capi.FN2_CORR_MFMA_BF16X3, "bf16x3", R.delta_bf16x3)):
            got = _maybe(lambda: _run_bwd(ad, bd, go, params, algo))
            if got is not None:
                _check(got[0], r1, dl(r1, ab1, n, C), f"{name} bwd md {md} {shape} family {fam} grad_input1")
                _check(got[1], r2, dl(r2, ab2, n, C), f"{name} bwd md {md} {shape} family {fam} grad_input2")


def test_fp32_mfma_subnormal_products(dev):
    """Operands near 2^-66: every product (2^-132) is an fp32 subnormal.  What v_mfma_f32_16x16x4_f32 does with them was not
    measured before; the header now states it (checked here against the fma chain's bracket, or against exact zeros if
    flushed)."""
    import fn2_capi
    shape = (1, 32, 8, 16)
    g = torch.Generator().manual_seed(5)
    a = (torch.randn(shape, generator=g) * 2.0 ** -66).to(dev)
    b = (torch.randn(shape, generator=g) * 2.0 ** -66).to(dev)
    ref = L.corr_fwd64(a, b, *CORR)
    absr = L.corr_fwd64(a.abs(), b.abs(), *CORR)
    out = _run_fwd(a, b, CORR, fn2_capi.FN2_CORR_MFMA_F32)
    assert bool((out != 0).any()), "fp32 MFMA flushes subnormal products to zero"
    _check(out, ref, R.delta_fma_chain(ref, absr, shape[1]), "fp32 MFMA subnormal products")


# ------------------------------------------------------------------ DIRECT fp32
@pytest.mark.parametrize("C", [1, 3])
def test_direct_f32(dev, C):
    import fn2_capi
    shape = (2, C, 13, 17)
    for params in ((3, 3, 4, 2, 2), (3, 3, 4, 1, 2)):
        B, _, H, W = shape
        nOut, oH, oW = L.out_shape(H, W, *params)
        for fam in (1, 2, 5, 7):
            a, b = R.family_inputs(fam, shape, seed=C + fam)
            ad, bd = a.to(dev), b.to(dev)
            out = _run_fwd(ad, bd, params, fn2_capi.FN2_CORR_AUTO)
            d = _run_fwd(ad, bd, params, fn2_capi.FN2_CORR_DIRECT)
            assert torch.equal(out.view(torch.int32), d.view(torch.int32))
            ref = L.corr_fwd64(ad, bd, *params)
            absr = L.corr_fwd64(ad.abs(), bd.abs(), *params)
            _check(out, ref, R.delta_direct_f32(ref, absr, C, params[1]), f"DIRECT fwd {params} {shape} family {fam}")
            if params[3] == 1:
                go = R.grad_output("normal", (B, nOut, oH, oW), fam).to(dev)
                g1, g2 = _run_bwd(ad, bd, go, params, fn2_capi.FN2_CORR_AUTO)
                d1, d2 = _run_bwd(ad, bd, go, params, fn2_capi.FN2_CORR_DIRECT)
                assert torch.equal(g1.view(torch.int32), d1.view(torch.int32)) and torch.equal(g2.view(torch.int32), d2.view(torch.int32))
                r1, r2 = L.corr_bwd64(ad, bd, go, *params)
                ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), go.abs(), *params)
                n = L.n_bwd(params[2], params[4], params[1])
                _check(g1, r1, R.delta_direct_bwd_f32(r1, ab1, n), f"DIRECT bwd {params} family {fam} grad_input1")
                _check(g2, r2, R.delta_direct_bwd_f32(r2, ab2, n), f"DIRECT bwd {params} family {fam} grad_input2")


# ------------------------------------------------------------------ float64
def test_f64_kernels(dev):
    """The fp64 MFMA kernel (AUTO at FlowNetC's configuration; an fp32-accumulating forward would leave its fp64 bracket, and its
    backward is told apart from the general kernel's, which accumulates in double too, by their results differing) and DIRECT
    double at C = 32 (outside the MFMA domain: AUTO == DIRECT): its forward accumulates in float as the reference does, its
    backward in double."""
    import fn2_capi
    for fam in (1, 2, 5, 6):
        shape = (3, 64, 10, 16)
        a, b = R.family_inputs(fam, shape, seed=fam)
        ad, bd = a.double().to(dev), b.double().to(dev)
        out = _run_fwd(ad, bd, CORR, fn2_capi.FN2_CORR_AUTO)
        ref = L.corr_fwd64(ad, bd, *CORR)
        absr = L.corr_fwd64(ad.abs(), bd.abs(), *CORR)
        _check(out, ref, R.delta_f64(ref, absr, shape[1]), f"fp64 MFMA fwd family {fam}", dtype=torch.float64)
        go = R.grad_output("normal", (3, 441, 10, 16), fam).double().to(dev)
        g1, g2 = _run_bwd(ad, bd, go, CORR, fn2_capi.FN2_CORR_AUTO)
        e1, e2 = _run_bwd(ad, bd, go, CORR, fn2_capi.FN2_CORR_DIRECT)
        assert not (torch.equal(g1, e1) and torch.equal(g2, e2)), "AUTO's double backward is the general kernel"
        r1, r2 = L.corr_bwd64(ad, bd, go, *CORR)
        ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), go.abs(), *CORR)
        _check(g1, r1, R.delta_f64(r1, ab1, 441), f"fp64 MFMA bwd family {fam} grad_input1", dtype=torch.float64)
        _check(g2, r2, R.delta_f64(r2, ab2, 441), f"fp64 MFMA bwd family {fam} grad_input2", dtype=torch.float64)
        _check(e1, r1, R.delta_direct_bwd_f64(r1, ab1, 441), f"DIRECT double bwd family {fam} grad_input1", dtype=torch.float64)
        _check(e2, r2, R.delta_direct_bwd_f64(r2, ab2, 441), f"DIRECT double bwd family {fam} grad_input2", dtype=torch.float64)
        shape = (3, 32, 10, 16)
        a, b = R.family_inputs(fam, shape, seed=fam)
        ad, bd = a.double().to(dev), b.double().to(dev)
        out = _run_fwd(ad, bd, CORR, fn2_capi.FN2_CORR_AUTO)
        d = _run_fwd(ad, bd, CORR, fn2_capi.FN2_CORR_DIRECT)
        assert torch.equal(out, d)
        ref = L.corr_fwd64(ad, bd, *CORR)
        absr = L.corr_fwd64(ad.abs(), bd.abs(), *CORR)
        # the float accumulator's result rounded to float is exact in double: the fp32 bracket, compared in double
        _check(out, ref, R.delta_direct_f32(ref, absr, 32), f"DIRECT double fwd family {fam}", dtype=torch.float64)
        g1, g2 = _run_bwd(ad, bd, go, CORR, fn2_capi.FN2_CORR_AUTO)
        e1, e2 = _run_bwd(ad, bd, go, CORR, fn2_capi.FN2_CORR_DIRECT)
        assert torch.equal(g1, e1) and torch.equal(g2, e2)
        r1, r2 = L.corr_bwd64(ad, bd, go, *CORR)
        ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), go.abs(), *CORR)
        _check(g1, r1, R.delta_direct_bwd_f64(r1, ab1, 441), f"DIRECT double bwd family {fam} grad_input1", dtype=torch.float64)
        _check(g2, r2, R.delta_direct_bwd_f64(r2, ab2, 441), f"DIRECT double bwd family {fam} grad_input2", dtype=torch.float64)
