"""CorrPyramid on the GPU (csrc/corr_pyramid.hip through libflownet2_hip_pyramid.so, corr_pyramid_cuda and the Python layer;
include/preview/flownet2_hip_pyramid.h).

1.  every level lies per element within the header's bound delta_l of the float64 reference (tests/corr_pyramid_ref.py), outputs
    pre-filled with NaN inside guarded allocations: every element written, nothing outside;
2.  levels >= 1 are bit-equal to the float32 pooling restatement applied to the kernel's own level 0;
3.  fn2y_corr_pyramid_fold is bit-equal to the float32 restatement: random gradients, a missing level, one-cell gradients;
4.  fmap1.grad and fmap2.grad through corr_pyramid by the rule of tests/pipelines_ref.py, the float32 composition beside them;
5.  the same through CorrBlock(fused_build=True), the default CorrBlock as the float32 composition;
6.  an inf in fmap1 and a NaN in fmap2: the non-finite elements are the float64 composition's, the others inside the bound;
7.  the bits repeat from run to run and on a side stream; the deterministic flag raises nothing;
8.  both entry points captured raw into a hipGraph, by the procedure of tests/test_gpu_capi_graph.py;
9.  half and bfloat16 maps through CorrBlock(fused_build=True); the refusals and their texts;
10. build forward and forward + backward are not slower than the PyTorch composition (the ratios are printed).

The largest error / bound seen is recorded in the docstring of test_forward_within_the_bound_and_fully_written and in DESIGN.md 4.19.
"""
import statistics
import warnings

import pytest
import torch

import corr_pyramid_ref as RP
import pipelines_ref as P
from test_gpu_corr_lookup import _guarded, _untouched, _windows

pytestmark = pytest.mark.gpu

_CACHE = {}


def _reference(shape):
    """The inputs and the float64 reference of one shape, computed once and shared (never modified)."""
    if shape not in _CACHE:
        B, C, (H, W), (H2, W2), L = shape
        f1, f2 = RP.inputs(shape, seed=7 + C)
        levels, S0 = RP.forward(f1, f2, L)
        _CACHE[shape] = (f1, f2, levels, RP.bounds(levels, S0, C))
    return _CACHE[shape]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.numel() == want.numel() and got.dtype == want.dtype == torch.float32, what
    n = int((_bits(got).reshape(-1) != _bits(want).reshape(-1)).sum())
    assert n == 0, f"{what}: {n} of {got.numel()} elements differ"


def _sizes(shape):
    B, C, (H, W), (H2, W2), L = shape
    return B, C, H, W, H2, W2, L, B * H * W


def _build(f1d, f2d, shape, off=0, what="forward"):
    """fn2y_corr_pyramid_forward into NaN-filled levels inside guarded allocations."""
    import fn2_capi
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    held = [_guarded((pixels, 1, H2 >> l, W2 >> l), f1d.device, off) for l in range(L)]
    fn2_capi.corr_pyramid_forward(f1d, f2d, L, out=[t for t, _ in held])
    for l, (t, whole) in enumerate(held):
        _untouched(whole, t, f"{what} level {l}")
    return [t for t, _ in held]


def _fold(grads, shape, off=0, what="fold"):
    import fn2_capi
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    G, whole = _guarded((pixels, H2, W2), next(g for g in grads if g is not None).device, off)
    fn2_capi.corr_pyramid_fold(grads, (B, C, H, W, H2, W2), out=G)
    _untouched(whole, G, what)
    assert not torch.isnan(G).any(), f"{what}: elements left unwritten"
    return G


def _grads(shape, seed):
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(pixels, 1, H2 >> l, W2 >> l, generator=g) for l in range(L)]


# ------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off1"])
@pytest.mark.parametrize("shape", RP.SHAPES, ids=RP.shape_id)
def test_forward_within_the_bound_and_fully_written(dev, shape, off):
    """Largest error / bound seen on one MI355X (level 0; the pooled levels lie below it): 2x40x9x11 0.0075, 1x256x21x28 0.0013,
    2x32x8x16-17x35 0.0097, 1x8x3x5-8x8 0.033, 2x64x16x32 0.0050."""
    f1, f2, levels, deltas = _reference(shape)
    got = _build(f1.to(dev), f2.to(dev), shape, off, RP.shape_id(shape))
    for l, t in enumerate(got):
        assert not torch.isnan(t).any(), f"level {l}: elements left unwritten"
    cpu = [t.cpu() for t in got]
    worst, per = RP.worst_ratio(cpu, levels, deltas)
    print(f"  {RP.shape_id(shape)} off {off}: error / bound per level " + " ".join(f"{r:.4f}" for r in per))
    assert not RP.misses(cpu, levels, deltas), f"{worst:.3g} x the bound"
    # levels >= 1 are the float32 pooling of the kernel's own level below, bit for bit
    for l in range(1, len(cpu)):
        _same_bits(cpu[l], RP.pool32(cpu[l - 1][:, 0]), f"level {l} against the pooling restatement")


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("shape", RP.SHAPES, ids=RP.shape_id)
def test_fold_has_the_bits_of_the_restatement(dev, shape):
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    variants = [("random", _grads(shape, 11), 0), ("random, offset pointers", _grads(shape, 12), 1)]
    for miss in range(L):
        g = _grads(shape, 13 + miss)
        g[miss] = None
        if any(t is not None for t in g):
            variants.append((f"level {miss} missing", g, 0))
    for l in range(L):      # one cell, the last one of its level: pins the level, the weight and the crop
        g = [torch.zeros(pixels, 1, H2 >> k, W2 >> k) for k in range(L)]
        g[l][pixels - 1, 0, (H2 >> l) - 1, (W2 >> l) - 1] = 3.0
        variants.append((f"one cell at level {l}", g, 0))
    for name, g, off in variants:
        want = RP.fold32(g, C, H2, W2)
        got = _fold([None if t is None else t.to(dev) for t in g], shape, off, name)
        _same_bits(got, want, f"{RP.shape_id(shape)} fold, {name}")
        if name.startswith("one cell"):
            l = int(name[-1])
            nz = got.cpu().nonzero()
            assert len(nz) == 4 ** l and bool((nz[:, 0] == pixels - 1).all())
            assert int(nz[:, 1].min()) == (((H2 >> l) - 1) << l) and int(nz[:, 2].min()) == (((W2 >> l) - 1) << l)


# ------------------------------------------------------------------ 4, 5
def _composed(f1, f2, L, gouts, dtype):
    a, b = f1.clone().to(dtype).requires_grad_(True), f2.clone().to(dtype).requires_grad_(True)
    pyr = RP.composition(a, b, L)
    torch.autograd.backward(pyr, [g.to(dtype) for g in gouts])
    return {"fmap1.grad": a.grad, "fmap2.grad": b.grad}


@pytest.mark.parametrize("shape", RP.SHAPES, ids=RP.shape_id)
def test_gradients_by_the_rule(dev, shape):
    from networks.correlation_package import corr_pyramid
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    f1, f2, _, _ = _reference(shape)
    gouts = _grads(shape, 21)
    o64, o32 = _composed(f1, f2, L, gouts, torch.float64), _composed(f1, f2, L, gouts, torch.float32)
    a, b = f1.to(dev).requires_grad_(True), f2.to(dev).requires_grad_(True)
    pyr = corr_pyramid(a, b, L)
    assert [tuple(t.shape) for t in pyr] == [(pixels, 1, H2 >> l, W2 >> l) for l in range(L)]
    torch.autograd.backward(pyr, [g.to(dev) for g in gouts])
    misses = P.rule_misses({"fmap1.grad": a.grad, "fmap2.grad": b.grad}, o32, o64, "corr_pyramid ")
    assert not misses, misses
    _, w1, w2 = RP.backward(f1, f2, gouts)       # the reference's own backward says the same as autograd through the composition
    assert float((w1 - o64["fmap1.grad"]).abs().max()) <= 1e-12 * float(w1.abs().max())
    assert float((w2 - o64["fmap2.grad"]).abs().max()) <= 1e-12 * float(w2.abs().max())


def test_through_corr_block(dev):
    import corr_sample_ref as RS
    from networks.correlation_package import CorrBlock
    shape = RP.SHAPES[1]
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    r = 3
    f1, f2, _, _ = _reference(shape)
    co = RS.coords("a", B, H, W, H2, W2, r, seed=3)
    go = torch.randn(B, L * (2 * r + 1) ** 2, H, W, generator=torch.Generator().manual_seed(4))

    def composed(dtype):
        import corr_lookup_ref as RL
        a, b = f1.clone().to(dtype).requires_grad_(True), f2.clone().to(dtype).requires_grad_(True)
        out = RL.compose(a, b, co.to(dtype), r, float(C) ** -0.5, num_levels=L)
        out.backward(go.to(dtype))
        return {"out": out.detach(), "fmap1.grad": a.grad, "fmap2.grad": b.grad}

    def block(fused):
        a, b = f1.to(dev).requires_grad_(True), f2.to(dev).requires_grad_(True)
        out = CorrBlock(a, b, num_levels=L, radius=r, fused_build=fused)(co.to(dev))
        out.backward(go.to(dev))
        return {"out": out.detach(), "fmap1.grad": a.grad, "fmap2.grad": b.grad}

    o64 = composed(torch.float64)
    misses = P.rule_misses(block(True), block(False), o64, "CorrBlock(fused_build=True) ")
    assert not misses, misses
    misses = P.rule_misses(block(True), composed(torch.float32), o64, "CorrBlock(fused_build=True), CPU float32 beside it ")
    assert not misses, misses


# ------------------------------------------------------------------ 6
def test_non_finite_inputs(dev):
    shape = RP.SHAPES[2]
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    f1, f2 = RP.inputs(shape, seed=31)
    f1[1, 3, 2, 5] = float("inf")
    f2[0, 7, 9, 20] = float("nan")
    levels, S0 = RP.forward(f1, f2, L)
    composed = RP.composition(f1.double(), f2.double(), L)
    got = [t.cpu() for t in _build(f1.to(dev), f2.to(dev), shape, 0, "non-finite")]
    finite0 = torch.isfinite(levels[0])
    deltas = RP.bounds([torch.where(finite0, levels[0], torch.zeros(()).double())] + levels[1:], torch.where(finite0, S0, torch.zeros(()).double()), C)
    for l, (g, w, c, d) in enumerate(zip(got, levels, composed, deltas)):
        g = g[:, 0]
        bad = ~torch.isfinite(c[:, 0])
        assert bool((bad == ~torch.isfinite(w)).all())
        assert 0 < int(bad.sum()) < bad.numel()
        assert bool((~torch.isfinite(g) == bad).all()), f"level {l}: the non-finite elements are not the float64 composition's"
        ok = ~bad
        assert bool(((g.double() - w).abs()[ok] <= d[ok]).all()), f"level {l}: a finite element misses the bound"


# ------------------------------------------------------------------ 7
def test_bits_repeat_and_deterministic_mode_is_silent(dev):
    from networks.correlation_package import corr_pyramid
    shape = RP.SHAPES[2]
    f1, f2, _, _ = _reference(shape)
    f1d, f2d = f1.to(dev), f2.to(dev)
    gr = [g.to(dev) for g in _grads(shape, 41)]
    first, G = _build(f1d, f2d, shape), _fold(gr, shape)
    for l, (a, b) in enumerate(zip(_build(f1d, f2d, shape), first)):
        _same_bits(a, b, f"second run, level {l}")
    _same_bits(_fold(gr, shape), G, "second fold")
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        side, sideG = _build(f1d, f2d, shape), _fold(gr, shape)
    s.synchronize()
    for l, (a, b) in enumerate(zip(side, first)):
        _same_bits(a, b, f"side stream, level {l}")
    _same_bits(sideG, G, "fold on a side stream")
    try:
        torch.use_deterministic_algorithms(True)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            pyr = corr_pyramid(f1d, f2d, shape[4])
    finally:
        torch.use_deterministic_algorithms(False)
    assert not caught, [str(w.message) for w in caught]
    for l, (a, b) in enumerate(zip(pyr, first)):
        _same_bits(a, b, f"deterministic mode, level {l}")


# ------------------------------------------------------------------ 8
def _graph_cases():
    import capi_graph_cases as G
    import fn2_capi
    shape = RP.SHAPES[2]
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    names = ["level%d" % l for l in range(L)]

    def maps(seed):
        f1, f2 = RP.inputs(shape, seed=100 + seed)
        return {"fmap1": f1, "fmap2": f2}

    def grads(seed):
        return {"grad_" + n: g for n, g in zip(names, _grads(shape, 200 + seed))}

    fwd = G.Case("fn2y_corr_pyramid_forward", ["fn2y_corr_pyramid_forward"], maps,
                 {n: G.Out((pixels, 1, H2 >> l, W2 >> l), torch.float32) for l, n in enumerate(names)},
                 lambda T: [G.raised(fn2_capi.corr_pyramid_forward(T["fmap1"], T["fmap2"], L, out=[T[n] for n in names]))])
    fold = G.Case("fn2y_corr_pyramid_fold", ["fn2y_corr_pyramid_fold"], grads, {"G": G.Out((pixels, H2, W2), torch.float32)},
                  lambda T: [G.raised(fn2_capi.corr_pyramid_fold([T["grad_" + n] for n in names], (B, C, H, W, H2, W2), out=T["G"]))])
    return [fwd, fold]


@pytest.mark.parametrize("which", [0, 1], ids=["fn2y_corr_pyramid_forward", "fn2y_corr_pyramid_fold"])
def test_entry_point_replays_from_a_hip_graph(dev, which):
    import capi_graph_cases as G
    from test_gpu_capi_graph import test_entry_point_replays_from_a_hip_graph as procedure
    case = _graph_cases()[which]
    assert case.id not in [c.id for c in G.CASES]       # built locally: that table is held to include/*.h
    procedure(dev, case)


# ------------------------------------------------------------------ 9
def test_doors(dev):
    import corr_pyramid_cuda
    import corr_sample_ref as RS
    from networks.correlation_package import CorrBlock, CorrPyramid, corr_pyramid
    shape = RP.SHAPES[0]
    B, C, H, W, H2, W2, L, pixels = _sizes(shape)
    f1, f2, _, _ = _reference(shape)
    f1d, f2d = f1.to(dev), f2.to(dev)
    want = _build(f1d, f2d, shape)
    for name, fn in (("forward_alloc", lambda: corr_pyramid_cuda.forward_alloc(f1d, f2d, L)), ("corr_pyramid", lambda: corr_pyramid(f1d, f2d, L)),
                     ("CorrPyramid", lambda: CorrPyramid(L)(f1d, f2d)), ("torch.ops.fn2.corr_pyramid", lambda: torch.ops.fn2.corr_pyramid(f1d, f2d, L))):
        for l, (a, b) in enumerate(zip(fn(), want)):
            _same_bits(a, b, f"{name}, level {l}")
    # more levels than one launch builds: pooled on from the fourth
    big = RP.SHAPES[4]
    g1, g2, _, _ = _reference(big)
    five = corr_pyramid(g1.to(dev), g2.to(dev), 5)
    assert [tuple(t.shape[2:]) for t in five] == [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)]
    # (avg_pool2d's own order of the three adds: three roundings of the block's absolute mean, as FN2Y_BOUND_PER_POOL counts them)
    below = five[3].cpu()[:, 0].double()
    assert bool(((five[4].cpu()[:, 0].double() - RP.pool_exact(below)).abs() <= 3 * 2.0 ** -24 * RP.pool_exact(below.abs())).all())
    # half and bfloat16 maps: CorrBlock widens them, as RAFT's .float()
    co = RS.coords("a", B, H, W, H2, W2, 2, seed=3).to(dev)
    for dtype in (torch.float16, torch.bfloat16):
        h1, h2 = f1d.to(dtype), f2d.to(dtype)
        narrow = CorrBlock(h1, h2, num_levels=L, radius=2, fused_build=True)
        for l, (a, b) in enumerate(zip(narrow.corr_pyramid, corr_pyramid(h1.float(), h2.float(), L))):
            _same_bits(a, b, f"{dtype} maps, level {l}")
        _same_bits(narrow(co), CorrBlock(h1.float(), h2.float(), num_levels=L, radius=2, fused_build=True)(co), f"{dtype} maps, lookup")
    # the refusals, in STATUS_PYRAMID's words
    einval = "flownet2_hip_pyramid: invalid shape, layout or parameter"
    with pytest.raises(RuntimeError, match=einval):
        corr_pyramid(f1d.transpose(2, 3).contiguous().transpose(2, 3), f2d, L)
    with pytest.raises(RuntimeError, match=einval):
        corr_pyramid(f1d, f2d, 0)
    with pytest.raises(RuntimeError, match=einval):
        corr_pyramid(f1d, f2d[:, :, :4].contiguous(), 4)          # 4 >> 3 == 0: the fourth level would be empty
    with pytest.raises(RuntimeError, match="flownet2_hip_pyramid: dtype not supported by this op"):
        corr_pyramid(f1d.half(), f2d.half(), L)
    with pytest.raises(RuntimeError, match="fmap2 has dtype"):
        corr_pyramid(f1d, f2d.half(), L)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_pyramid(f1, f2, L)


# ------------------------------------------------------------------ 10
def test_not_slower_than_the_composition(dev):
    """2 x 64 x 48 x 64, L = 4 (a 75 MB volume), medians over 5 alternating windows of 10 calls.  Only "not slower" is asserted, the
    build forward and the build forward + backward each against the PyTorch composition; the ratios are printed (DESIGN.md 4.19 and
    profiles/corr_pyramid_micro.json record the bench script's)."""
    from networks.correlation_package import corr_pyramid
    B, C, H, W, L = 2, 64, 48, 64, 4
    g = torch.Generator().manual_seed(1)
    f1, f2 = torch.randn(B, C, H, W, generator=g).to(dev), torch.randn(B, C, H, W, generator=g).to(dev)
    with torch.no_grad():
        ours, ref = corr_pyramid(f1, f2, L), RP.composition(f1, f2, L)
        for a, b in zip(ours, ref):
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())      # the same function; tests 1 - 6 pin the precision
        tf, tc = _windows([lambda: corr_pyramid(f1, f2, L), lambda: RP.composition(f1, f2, L)])
    del ours, ref
    mf, mc = statistics.median(tf), statistics.median(tc)
    print(f"  CorrPyramid build forward {mf * 1e3:.1f} us, composition {mc * 1e3:.1f} us: {mc / mf:.2f} x")
    gouts = [torch.randn(B * H * W, 1, H >> l, W >> l, device=dev) for l in range(L)]
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)

    def train(build):
        torch.autograd.backward(build(a, b, L), gouts)
        a.grad = b.grad = None

    tb, tcb = _windows([lambda: train(corr_pyramid), lambda: train(RP.composition)])
    mb, mcb = statistics.median(tb), statistics.median(tcb)
    print(f"  CorrPyramid build forward + backward {mb * 1e3:.1f} us, composition {mcb * 1e3:.1f} us: {mcb / mb:.2f} x")
    assert mf <= mc, (tf, tc)
    assert mb <= mcb, (tb, tcb)
