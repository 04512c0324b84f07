"""The split-operand matrix kernels against their bounds with n = n_nz, on sparse inputs (tests/split_terms_ref.py; the host side:
tests/test_split_terms_host.py).

The seven kernels that form an fp32 product from several low-precision partial products -- bf16x3: corr_fwd_mfma_bf16x3,
corr_bwd_mfma_bf16x3, pyramid_fwd; f16x2: the narrow and column-window forward and backward -- run through the C-ABI helpers on
inputs whose output elements have 0 .. 4 non-zero terms.  Every element must lie in the fp32 bracket of its float64 reference
widened by the documented bound with the term count n replaced by the element's n_nz, which is 10 .. 400 times tighter than
with all terms and below the size of one small partial product; where n_nz = 0 the element must be +0 bit for bit.  Outputs are
prefilled with NaN, the explicit selector is bit-equal to AUTO where AUTO picks that kernel, and the worst error / bound is
printed (recorded in each test's docstring and in DESIGN.md 4.22).
"""
import pytest
import torch

import corr_pyramid_ref as RP
import lowp_ref as L
import split_terms_ref as T
from test_gpu_corr_pyramid import _build, _same_bits
from test_gpu_f32_contract import _check, _run_bwd, _run_fwd

pytestmark = pytest.mark.gpu

CORR = L.CORR
sid = lambda s: "x".join(map(str, s))


def _bits_equal(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def _auto_is(direction, shape, params, kernel):
    """Whether the dispatcher's first kernel for this float32 call is `kernel` (fn2_capi.CORR_KERNELS; the bf16x3 kernels are the
    MFMA_F32 entry's own first choice)."""
    import fn2_capi
    return fn2_capi.correlation_plan(direction, fn2_capi.FN2_F32, shape, *params)[0] == kernel


# ------------------------------------------------------------------ bf16x3 Correlation forward
@pytest.mark.parametrize("md", T.X3_FWD_MD)
@pytest.mark.parametrize("shape", T.X3_FWD_SHAPES, ids=sid)
def test_bf16x3_forward(dev, shape, md):
    """Largest error / n_nz bound seen on one MI355X: (1, 32, 8, 16) 0.495, (1, 64, 8, 20) 0.501, (2, 96, 12, 64) 0.548, at md 20 and md 12 alike
    (the sequential-fp32 model: 0.495, 0.501, 0.54)."""
    import fn2_capi
    params = T.params_md(md)
    C = shape[1]
    auto_is_x3 = _auto_is("forward", shape, params, "MFMA_F32")
    worst = 0.0
    for name, a, b in T.x3_fwd_inputs(shape):
        what = f"bf16x3 fwd md {md} {shape} {name}"
        ad, bd = a.to(dev), b.to(dev)
        out = _run_fwd(ad, bd, params, fn2_capi.FN2_CORR_MFMA_BF16X3)
        if auto_is_x3:
            assert _bits_equal(out, _run_fwd(ad, bd, params, fn2_capi.FN2_CORR_AUTO)), f"{what}: AUTO is not the bf16x3 kernel"
        ref = L.corr_fwd64(ad, bd, *params)
        absr = L.corr_fwd64(ad.abs(), bd.abs(), *params)
        n = T.nnz_fwd(ad, bd, params)
        assert int(n.max()) >= 1
        worst = max(worst, _check(out, ref, T.delta_x3(ref, absr, n, C), what))
        assert T.plus_zero_where(out, n), f"{what}: an element without a non-zero term is not +0"
    print(f"  bf16x3 fwd md {md} {shape}: worst error / n_nz bound {worst:.3g} (AUTO {'is' if auto_is_x3 else 'is not'} this kernel)")


# ------------------------------------------------------------------ bf16x3 Correlation backward
@pytest.mark.parametrize("shape", T.X3_BWD_SHAPES, ids=sid)
def test_bf16x3_backward(dev, shape):
    """Largest error / n_nz bound seen on one MI355X: (1, 64, 8, 20) 0.501, (1, 128, 12, 36) 0.515."""
    import fn2_capi
    C = shape[1]
    auto_is_x3 = _auto_is("backward", shape, CORR, "MFMA_F32")
    worst = 0.0
    for name, a, b, go in T.x3_bwd_inputs(shape):
        what = f"bf16x3 bwd {shape} {name}"
        ad, bd, gd = a.to(dev), b.to(dev), go.to(dev)
        got = _run_bwd(ad, bd, gd, CORR, fn2_capi.FN2_CORR_MFMA_BF16X3)
        if auto_is_x3:
            auto = _run_bwd(ad, bd, gd, CORR, fn2_capi.FN2_CORR_AUTO)
            assert _bits_equal(got[0], auto[0]) and _bits_equal(got[1], auto[1]), f"{what}: AUTO is not the bf16x3 kernel"
        refs = L.corr_bwd64(ad, bd, gd, *CORR)
        sums = L.corr_bwd64(ad.abs(), bd.abs(), gd.abs(), *CORR)
        ns = T.nnz_bwd(ad, bd, gd, CORR)
        for which, g, r, s, n in zip((1, 2), got, refs, sums, ns):
            assert 1 <= int(n.max()) < 441
            worst = max(worst, _check(g, r, T.delta_x3(r, s, n, C), f"{what} grad_input{which}"))
            assert T.plus_zero_where(g, n), f"{what} grad_input{which}: an element without a non-zero term is not +0"
    print(f"  bf16x3 bwd {shape}: worst error / n_nz bound {worst:.3g}")


# ------------------------------------------------------------------ the pyramid
@pytest.mark.parametrize("shape", RP.SHAPES, ids=RP.shape_id)
def test_pyramid(dev, shape):
    """Largest error / n_nz bound seen on one MI355X (level 0; the pooled levels lie below it): 2x40x9x11 0.547,
    1x256x21x28 0.555, 2x32x8x16-17x35 0.570, 1x8x3x5-8x8 0.497, 2x64x16x32 0.556."""
    B, C, (H, W), (H2, W2), Lv = shape
    worst = 0.0
    for name, f1, f2 in T.pyramid_inputs(shape):
        what = f"pyramid {RP.shape_id(shape)} {name}"
        levels, S0 = RP.forward(f1, f2, Lv)
        n = T.nnz_pyramid(f1, f2)
        deltas = T.pyramid_bounds(levels, S0, C, n)
        got = _build(f1.to(dev), f2.to(dev), shape, 0, what)
        for l, t in enumerate(got):
            assert not torch.isnan(t).any(), f"{what} level {l}: elements left unwritten"
        cpu = [t.cpu() for t in got]
        ratio, per = RP.worst_ratio(cpu, levels, deltas)
        print(f"  {what}: error / n_nz bound per level " + " ".join(f"{r:.3g}" for r in per))
        assert not RP.misses(cpu, levels, deltas), f"{what}: {ratio:.3g} x the n_nz bound"
        for l, (t, c) in enumerate(zip(cpu, T.pooled_counts(n, Lv))):
            assert T.plus_zero_where(t[:, 0], c), f"{what} level {l}: an element without a non-zero term is not +0"
        for l in range(1, Lv):
            _same_bits(cpu[l], RP.pool32(cpu[l - 1][:, 0]), f"{what} level {l} against the pooling restatement")
        worst = max(worst, ratio)
    print(f"  pyramid {RP.shape_id(shape)}: worst error / n_nz bound {worst:.3g}")


# ------------------------------------------------------------------ f16x2 forward
@pytest.mark.parametrize("shape", [T.F16_FWD_NARROW, T.F16_FWD_WIDE], ids=["narrow", "wide"])
def test_f16x2_forward(dev, shape):
    """Largest error / n_nz bound seen on one MI355X: narrow (1, 320, 6, 56) 0.086, wide (1, 320, 2, 136) 0.116."""
    import fn2_capi
    a, b = T.f16_fwd_inputs(shape)
    ad, bd = a.to(dev), b.to(dev)
    out = _run_fwd(ad, bd, CORR, fn2_capi.FN2_CORR_MFMA_F16X2)
    assert _auto_is("forward", shape, CORR, "F16X2")
    assert _bits_equal(out, _run_fwd(ad, bd, CORR, fn2_capi.FN2_CORR_AUTO)), f"{shape}: AUTO is not the f16x2 kernel"
    ref, delta, n = T.fwd_f16x2(ad, bd, wide=shape[3] > 64)
    _check(out, ref, delta, f"f16x2 fwd {shape} channel_sparse")
    assert T.plus_zero_where(out, n), f"{shape}: an element without a non-zero term is not +0"


# ------------------------------------------------------------------ f16x2 backward
@pytest.mark.parametrize("shape", T.F16_BWD_SHAPES, ids=sid)
def test_f16x2_backward(dev, shape):
    """Largest error / n_nz bound seen on one MI355X: (1, 64, 2, 8) 0.241, (9, 192, 6, 56) 0.163, (1, 64, 6, 72) 0.154,
    (22, 64, 48, 8) 0.168 (the larger of the two gradients)."""
    import fn2_capi
    a, b, go = T.f16_bwd_inputs(shape)
    ad, bd, gd = a.to(dev), b.to(dev), go.to(dev)
    got = _run_bwd(ad, bd, gd, CORR, fn2_capi.FN2_CORR_MFMA_F16X2)
    assert _auto_is("backward", shape, CORR, "F16X2")
    auto = _run_bwd(ad, bd, gd, CORR, fn2_capi.FN2_CORR_AUTO)
    assert _bits_equal(got[0], auto[0]) and _bits_equal(got[1], auto[1]), f"{shape}: AUTO is not the f16x2 kernel"
    for which, g, (r, d, n) in zip((1, 2), got, T.bwd_f16x2(ad, bd, gd)):
        _check(g, r, d, f"f16x2 bwd {shape} grad_sparse grad_input{which}")
        assert T.plus_zero_where(g, n), f"{shape} grad_input{which}: an element without a non-zero term is not +0"
