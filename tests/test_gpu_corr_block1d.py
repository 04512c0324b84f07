"""CorrSample1d / CorrBlock1D on the GPU (csrc/corr_sample1d.hip through libflownet2_hip_sample1d.so, corr_sample1d_cuda and the Python
layer; include/staging/flownet2_hip_sample1d.h).

1. forward and backward lie per element within the header's bound of the float64 reference (tests/corr_sample1d_ref.py), no element
   left out, over the level widths (21, 10, 5, 2), (19,), (1,) * 8 and (3, 40), r in {0, 1, 4, 8}, pointer offsets of 0 and 1 element
   and every coordinate family; the gradient has the bits of +0 outside the window and everywhere for a pixel without taps;
2. a B x 2 x H x W coordinate tensor whose channel 1 is NaN gives the bits of the B x 1 x H x W call;
3. the bits repeat over three runs and on a side stream; under torch.use_deterministic_algorithms(True) nothing is raised or warned;
4. CorrBlock1D against the float64 composition on the CPU (build + lookup) by the rule of DESIGN.md 4.16 (tests/pipelines_ref.py):
   the output and both feature gradients;
5. the eager node, the static forward / backward, torch.ops.fn2.corr_sample1d and a torch.compile'd call give the same bits;
6. both entry points captured raw into a hipGraph, by the procedure of tests/test_gpu_capi_graph.py;
7. forward and backward are not slower than the composition's lookup on the same pyramid (the ratios are printed).

Every output sits inside a larger allocation filled with a sentinel that must be untouched afterwards, and is pre-filled with NaN.
"""
import statistics
import warnings

import numpy as np
import pytest
import torch

import corr_sample1d_ref as R
import pipelines_ref as P

QUERY = ((2, 3, 37), (1, 1, 1), (2, 2, 64))     # ragged against any pixel tile; one pixel; whole tiles
POOLED, ONE, EIGHT, UNRELATED = (21, 10, 5, 2), (19,), (1,) * 8, (3, 40)
# (B, H, W), the level widths, r, coordinate family, pointer offset in elements
CASES = [
    (QUERY[0], POOLED, 4, "a", 0), (QUERY[0], POOLED, 1, "b", 1), (QUERY[0], POOLED, 0, "c", 1), (QUERY[0], POOLED, 8, "g", 0),
    (QUERY[0], POOLED, 8, "e", 1), (QUERY[0], POOLED, 4, "c", 0), (QUERY[0], POOLED, 4, "d", 1),
    (QUERY[0], ONE, 4, "e", 1), (QUERY[0], ONE, 1, "d", 0), (QUERY[0], ONE, 0, "b", 1), (QUERY[0], ONE, 8, "c", 0),
    (QUERY[0], EIGHT, 1, "c", 0), (QUERY[0], EIGHT, 4, "b", 1), (QUERY[0], UNRELATED, 4, "e", 1), (QUERY[0], UNRELATED, 0, "a", 0),
    (QUERY[0], UNRELATED, 8, "b", 0), (QUERY[0], UNRELATED, 1, "g", 1),
    (QUERY[1], POOLED, 1, "e", 0), (QUERY[1], EIGHT, 8, "b", 1), (QUERY[1], ONE, 4, "a", 1), (QUERY[1], UNRELATED, 0, "c", 0),
    (QUERY[2], POOLED, 4, "d", 0), (QUERY[2], ONE, 0, "g", 0), (QUERY[2], EIGHT, 4, "e", 1), (QUERY[2], POOLED, 8, "c", 1),
    (QUERY[2], POOLED, 1, "a", 0), (QUERY[2], POOLED, 4, "g", 1), (QUERY[2], UNRELATED, 0, "b", 1), (QUERY[2], UNRELATED, 8, "a", 0),
]
assert {c[3] for c in CASES} == set(R.FAMILIES) and {c[2] for c in CASES} == {0, 1, 4, 8} and {c[0] for c in CASES} == set(QUERY)
assert {c[1] for c in CASES} == {POOLED, ONE, EIGHT, UNRELATED} and {c[4] for c in CASES} == {0, 1}
WORST = {}


def _case_id(c):
    return "%dx%dx%d-W2_%s-r%d-%s-off%d" % (*c[0], "_".join(map(str, c[1][:4])) + ("_x%d" % len(c[1]) if len(c[1]) > 4 else ""), c[2], c[3], c[4])


def _normal(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def _inputs(B, H, W, widths, r, fam, seed):
    levels = [_normal((B * H * W, 1, 1, w), seed + 10 * l) for l, w in enumerate(widths)]
    co = R.coords(fam, B, H, W, widths[0], r, seed)
    go = _normal((B, len(widths) * (2 * r + 1), H, W), seed + 5)
    return levels, co, go


def _fwd(levels, co, r, off=0, what="forward"):
    import fn2_capi
    from test_gpu_corr_lookup import _guarded, _untouched
    B, _, H, W = co.shape
    out, whole = _guarded((B, len(levels) * (2 * r + 1), H, W), co.device, off)
    fn2_capi.corr_sample1d_forward(levels, co, r, out=out)
    _untouched(whole, out, what)
    assert not torch.isnan(out).any(), f"{what}: elements left unwritten"
    return out


def _bwd(levels, co, go, r, off=0, what="backward"):
    import fn2_capi
    from test_gpu_corr_lookup import _guarded, _untouched
    held = [_guarded(t.shape, co.device, off) for t in levels]
    fn2_capi.corr_sample1d_backward(levels, co, go, r, out=[g for g, _ in held])
    for l, (g, whole) in enumerate(held):
        _untouched(whole, g, f"{what} level {l}")
        assert not torch.isnan(g).any(), f"{what}: elements of level {l} left unwritten"
    return [g for g, _ in held]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    n = int((_bits(got) != _bits(want)).sum())
    assert n == 0, f"{what}: {n} of {got.numel()} elements differ"


def _ratio(got, exact, S, what):
    """Every element against the header's bound; the largest error / bound."""
    err, delta = np.abs(got.detach().cpu().numpy().astype(np.float64).reshape(exact.shape) - exact), R.bound(S)
    ratio = float((err / delta).max())
    print(f"  {what}: error / bound {ratio:.3f}")
    assert (err <= delta).all(), f"{what}: {ratio:.3g} x the bound"
    return ratio


# ------------------------------------------------------------------ 1
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_within_the_headers_bound_and_fully_written(dev, case):
    (B, H, W), widths, r, fam, off = case
    what = _case_id(case)
    levels, co, go = _inputs(B, H, W, widths, r, fam, seed=3 * r + W + len(widths))
    exact, S = R.forward([t.numpy() for t in levels], co.numpy(), r)
    ref = R.backward(widths, co.numpy(), go.numpy(), r)
    lv, cod, god = [t.to(dev) for t in levels], co.to(dev), go.to(dev)
    out = _fwd(lv, cod, r, off, what)
    grads = _bwd(lv, cod, god, r, off, what)
    ratios = [_ratio(out, exact, S, what + " forward")] + [_ratio(g, e, Sg, f"{what} gradient of level {l}")
                                                          for l, (g, (e, Sg, _)) in enumerate(zip(grads, ref))]
    WORST[fam] = max(WORST.get(fam, 0.0), *ratios)
    print(f"  {what}: error / bound forward {ratios[0]:.3f}, backward {max(ratios[1:]):.3f}; family {fam} so far {WORST[fam]:.3f}")
    # exactly +0 where the reference has no term: outside the window, outside the level's reach, pixels without taps
    assert bool((_bits(out).cpu()[torch.from_numpy(S == 0)] == 0).all()), what + ": forward not +0 where no term arrives"
    for l, (g, (_, _, n)) in enumerate(zip(grads, ref)):
        assert bool((_bits(g).cpu().reshape(n.shape)[torch.from_numpy(n == 0)] == 0).all()), f"{what}: level {l} not +0 outside the window"
    ok = torch.from_numpy(R.has_taps(co.numpy()))
    if fam == "g":
        assert not bool(ok.all())
        gone = ~ok
        assert bool((_bits(out).cpu().permute(0, 2, 3, 1)[gone] == 0).all()), what + ": a pixel without taps is not +0"
        for g in grads:
            assert bool((_bits(g).cpu().reshape((B, H, W, -1))[gone] == 0).all()), what + ": a gradient slice without taps is not +0"
    else:
        assert bool(ok.all())
    if fam == "d":
        assert bool((S == 0).all()) and all(bool((n == 0).all()) for _, _, n in ref)
    elif B * H * W > 1:
        assert float(np.abs(exact).max()) > 0 and any(int(n.max()) > 0 for _, _, n in ref), what + ": a trivial case"


# ------------------------------------------------------------------ 2
@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["e", "g"])
def test_the_y_channel_is_never_read(dev, fam):
    (B, H, W), widths, r = QUERY[0], POOLED, 4
    levels, co, go = _inputs(B, H, W, widths, r, fam, seed=17)
    lv, god = [t.to(dev) for t in levels], go.to(dev)
    one = co.to(dev)
    two = torch.cat([one, torch.full_like(one, float("nan"))], dim=1).contiguous()
    assert two.shape == (B, 2, H, W) and two.stride(0) == 2 * H * W and bool(torch.isnan(two[:, 1]).all())
    want, wgrads = _fwd(lv, one, r), _bwd(lv, one, god, r)
    _same_bits(_fwd(lv, two, r), want, "B x 2 x H x W, forward")
    for l, (g, w) in enumerate(zip(_bwd(lv, two, god, r), wgrads)):
        _same_bits(g, w, f"B x 2 x H x W, gradient of level {l}")
    from networks.correlation_package import corr_sample1d
    leaves = [t.clone().requires_grad_(True) for t in lv]
    out = corr_sample1d(leaves, two, r)
    _same_bits(out.detach(), want, "corr_sample1d on B x 2 x H x W")
    out.backward(god)
    for l, (t, w) in enumerate(zip(leaves, wgrads)):
        _same_bits(t.grad, w, f"corr_sample1d on B x 2 x H x W, gradient of level {l}")


# ------------------------------------------------------------------ 3
@pytest.mark.gpu
def test_bits_repeat_and_deterministic_mode_is_silent(dev):
    from networks.correlation_package import corr_sample1d
    (B, H, W), widths, r = QUERY[0], POOLED, 4
    levels, co, go = _inputs(B, H, W, widths, r, "a", seed=11)
    lv, cod, god = [t.to(dev) for t in levels], co.to(dev), go.to(dev)
    out, grads = _fwd(lv, cod, r), _bwd(lv, cod, god, r)
    for run in (2, 3):
        _same_bits(_fwd(lv, cod, r), out, f"forward, run {run}")
        for g, w in zip(_bwd(lv, cod, god, r), grads):
            _same_bits(g, w, f"backward, run {run}")
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        so, sg = _fwd(lv, cod, r), _bwd(lv, cod, god, r)
    s.synchronize()
    _same_bits(so, out, "forward on a side stream")
    for g, w in zip(sg, grads):
        _same_bits(g, w, "backward on a side stream")
    try:
        torch.use_deterministic_algorithms(True)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            leaves = [t.clone().requires_grad_(True) for t in lv]
            o = corr_sample1d(leaves, cod, r)
            o.backward(god)
    finally:
        torch.use_deterministic_algorithms(False)
    assert not caught, [str(w.message) for w in caught]
    _same_bits(o.detach(), out, "deterministic mode, forward")
    for t, w in zip(leaves, grads):
        _same_bits(t.grad, w, "deterministic mode, backward")


# ------------------------------------------------------------------ 4
def block_case():
    """B = 2, C = 16, H = 3, W1 = 37, W2 = 41, L = 4, r = 4: the maps, RAFT-Stereo's B x 2 x H x W coordinates, grad_out (CPU)."""
    B, C, H, W1, W2, L, r = 2, 16, 3, 37, 41, 4, 4
    f1, f2 = _normal((B, C, H, W1), 1), _normal((B, C, H, W2), 2)
    cx = R.coords("a", B, H, W1, W2, r, seed=3)
    co = torch.cat([cx, torch.arange(H, dtype=torch.float32).view(1, 1, H, 1).expand(B, 1, H, W1)], dim=1).contiguous()
    return {"f1": f1, "f2": f2, "co": co, "go": _normal((B, L * (2 * r + 1), H, W1), 4), "L": L, "r": r}


def composed(case, dtype):
    """RAFT-Stereo's composition, build and lookup, on the CPU in ``dtype``: the output and both feature gradients."""
    a, b = case["f1"].clone().to(dtype).requires_grad_(True), case["f2"].clone().to(dtype).requires_grad_(True)
    out = R.compose(a, b, case["co"].to(dtype), case["L"], case["r"])
    out.backward(case["go"].to(dtype))
    return {"out": out.detach(), "fmap1.grad": a.grad, "fmap2.grad": b.grad}


@pytest.mark.gpu
def test_corr_block1d_against_the_float64_composition(dev):
    from networks.correlation_package import CorrBlock1D
    case = block_case()
    o64, o32 = composed(case, torch.float64), composed(case, torch.float32)
    a, b = case["f1"].to(dev).requires_grad_(True), case["f2"].to(dev).requires_grad_(True)
    block = CorrBlock1D(a, b, num_levels=case["L"], radius=case["r"])
    assert [tuple(t.shape) for t in block.corr_pyramid] == [(2 * 3 * 37, 1, 1, w) for w in (41, 20, 10, 5)]
    out = block(case["co"].to(dev))
    assert out.shape == (2, 4 * 9, 3, 37) and out.dtype == torch.float32 and out.is_contiguous()
    out.backward(case["go"].to(dev))
    misses = P.rule_misses({"out": out.detach(), "fmap1.grad": a.grad, "fmap2.grad": b.grad}, o32, o64, "CorrBlock1D ")
    assert not misses, misses
    assert float(o64["out"].abs().max()) > 0.1 and float(o64["fmap1.grad"].abs().max()) > 0.1 and float(o64["fmap2.grad"].abs().max()) > 0.1


# ------------------------------------------------------------------ 5
@pytest.mark.gpu
def test_every_door_gives_the_same_bits(dev):
    import torch._dynamo

    import corr_sample1d_cuda
    from networks.correlation_package import CorrSample1d, CorrSample1dFunction, corr_sample1d
    (B, H, W), widths, r = QUERY[0], POOLED, 4
    levels, co, go = _inputs(B, H, W, widths, r, "a", seed=21)
    lv, cod, god = [t.to(dev) for t in levels], co.to(dev), go.to(dev)
    want, wgrads = _fwd(lv, cod, r), _bwd(lv, cod, god, r)
    _same_bits(corr_sample1d_cuda.forward_alloc(lv, cod, r), want, "forward_alloc")
    for g, w in zip(corr_sample1d_cuda.backward_alloc(cod, god, list(widths), [4] * len(widths), r), wgrads):
        _same_bits(g, w, "backward_alloc")

    def static(p, c):      # torch's own Function.apply: it drives the static forward / backward
        return super(CorrSample1dFunction, CorrSample1dFunction).apply(c, r, *p)

    torch._dynamo.reset()
    doors = (("corr_sample1d_cuda.apply", lambda p, c: corr_sample1d_cuda.apply(p, c, r)), ("corr_sample1d", lambda p, c: corr_sample1d(p, c, r)),
             ("CorrSample1d", CorrSample1d(r)), ("static forward / backward", static),
             ("torch.ops.fn2.corr_sample1d", lambda p, c: torch.ops.fn2.corr_sample1d(p, c, r)),
             ("torch.compile", torch.compile(lambda p, c: corr_sample1d(p, c, r), backend="aot_eager", fullgraph=True)))
    for name, fn in doors:
        leaves = [t.clone().requires_grad_(True) for t in lv]
        out = fn(leaves, cod)
        _same_bits(out.detach(), want, name)
        out.backward(god)
        for t, w in zip(leaves, wgrads):
            _same_bits(t.grad, w, name + " backward")
    with pytest.raises(RuntimeError, match=r"pass coords\.detach\(\)"):
        corr_sample1d([t.clone().requires_grad_(True) for t in lv], cod.clone().requires_grad_(True), r)
    with pytest.raises(RuntimeError, match="radius 9 outside 0 .. 8"):
        corr_sample1d_cuda.forward_alloc(lv, cod, 9)
    with pytest.raises(RuntimeError, match=r"float32 tensors expected, got .*use \.float\(\)"):
        corr_sample1d_cuda.forward_alloc([t.half() for t in lv], cod, r)
    with pytest.raises(RuntimeError, match=r"a pyramid level has shape \[111, 1, 1, 21\], expected \[222, 1, 1, W2\] or \[222, W2\]"):
        corr_sample1d_cuda.forward_alloc([lv[0][:111]], cod, r)
    with pytest.raises(RuntimeError, match=r"gradOutput has shape .*expected \[2, 36, 3, 37\]"):
        corr_sample1d_cuda.backward_alloc(cod, god[:, :9], list(widths), [4] * len(widths), r)
    with pytest.raises(RuntimeError, match="the pyramid has 9 levels, expected 1 .. 8"):       # the binding itself, not the fake operator
        corr_sample1d_cuda.forward_alloc([lv[0]] * 9, cod, r)
    with pytest.raises(RuntimeError, match="the pyramid has 9 levels, expected 1 .. 8"):
        corr_sample1d_cuda.backward_alloc(cod, god, [21] * 9, [4] * 9, r)
    with pytest.raises(RuntimeError, match="level 1 has 3 dimensions"):
        corr_sample1d_cuda.backward_alloc(cod, god, list(widths), [4, 3, 4, 4], r)
    # the node keeps coords and the levels' shapes for its backward, not the levels: freeing them costs it nothing
    leaves = [t.clone().requires_grad_(True) for t in lv]
    for name, fn in doors[:5]:
        levels = [t * 1.0 for t in leaves]           # not leaves, and held by nothing else: mul by a scalar saves no tensor
        out = fn(levels, cod)
        torch.cuda.synchronize()
        held, nbytes = torch.cuda.memory_allocated(dev), sum(4 * t.numel() for t in levels)
        del levels
        assert held - torch.cuda.memory_allocated(dev) >= nbytes, f"{name}: the autograd graph keeps the pyramid alive"
        out.backward(god)
        for t, w in zip(leaves, wgrads):
            _same_bits(t.grad, w, name + " backward after the levels were freed")
            t.grad = None
    # levels as (P, W2), and non-contiguous coordinates
    _same_bits(corr_sample1d([t.view(t.shape[0], -1) for t in lv], cod, r), want, "levels as (P, W2)")
    cnc = cod.transpose(2, 3).contiguous().transpose(2, 3)
    assert not cnc.is_contiguous()
    _same_bits(corr_sample1d(lv, cnc, r), want, "non-contiguous coordinates")


# ------------------------------------------------------------------ 6
def _graph_cases():
    import capi_graph_cases as G
    import fn2_capi
    (B, H, W), widths, r = (2, 3, 19), POOLED, 3
    names = ["level%d" % l for l in range(len(widths))]
    oshape = (B, len(widths) * (2 * r + 1), H, W)

    def inputs(seed, gout=False):
        levels, co, go = _inputs(B, H, W, widths, r, "a", seed=100 + seed)
        d = {"coords": torch.cat([co, torch.full_like(co, float("nan"))], dim=1)}       # RAFT-Stereo's layout; y is never read
        if gout:
            d["grad_out"] = go
        else:
            d.update(zip(names, levels))
        return d

    fwd = G.Case("fn2h_corr_sample1d_forward", ["fn2h_corr_sample1d_forward"], inputs, {"out": G.Out(oshape, torch.float32)},
                 lambda T: [G.raised(fn2_capi.corr_sample1d_forward([T[n] for n in names], T["coords"], r, out=T["out"]))])
    bwd = G.Case("fn2h_corr_sample1d_backward", ["fn2h_corr_sample1d_backward"], lambda seed: inputs(seed, gout=True),
                 {"grad_" + n: G.Out((B * H * W, 1, 1, w), torch.float32) for n, w in zip(names, widths)},
                 lambda T: [G.raised(fn2_capi.corr_sample1d_backward([T["grad_" + n] for n in names], T["coords"], T["grad_out"], r,
                                                                     out=[T["grad_" + n] for n in names]))])
    return [fwd, bwd]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1], ids=["fn2h_corr_sample1d_forward", "fn2h_corr_sample1d_backward"])
def test_entry_point_replays_from_a_hip_graph(dev, which):
    import capi_graph_cases as G
    from test_gpu_capi_graph import test_entry_point_replays_from_a_hip_graph as procedure
    case = _graph_cases()[which]
    assert case.id not in [c.id for c in G.CASES]       # built locally: that table is held to include/*.h
    procedure(dev, case)


# ------------------------------------------------------------------ 7
@pytest.mark.gpu
def test_not_slower_than_the_composition(dev):
    """B = 2, H x W1 = 40 x 90, W2 = 90, L = 4, r = 4, smooth coordinates, medians over 5 alternating windows of 10 calls.  Only "not
    slower" is asserted, forward and backward each against the composition's on the same pyramid; the ratios are printed
    (DESIGN.md 4.21 and profiles/corr_block1d_micro.json record the bench script's)."""
    from networks.correlation_package import CorrBlock1D, corr_sample1d
    from test_gpu_corr_lookup import _windows
    B, C, H, W1, W2, L, r = 2, 32, 40, 90, 90, 4, 4
    block = CorrBlock1D(_normal((B, C, H, W1), 1).to(dev), _normal((B, C, H, W2), 2).to(dev), num_levels=L, radius=r)
    cx = R.coords("a", B, H, W1, W2, r, seed=4)
    co = torch.cat([cx, torch.zeros_like(cx)], dim=1).to(dev)
    go = _normal((B, L * (2 * r + 1), H, W1), 5).to(dev)
    with torch.no_grad():
        ref, out = R.compose_lookup(block.corr_pyramid, co, r), block(co)
        assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max())       # the same function; tests 1 - 4 pin the precision
        tl, tc = _windows([lambda: block(co), lambda: R.compose_lookup(block.corr_pyramid, co, r)])
    ml, mc = statistics.median(tl), statistics.median(tc)
    print(f"  CorrBlock1D lookup forward {ml * 1e3:.1f} us, composition {mc * 1e3:.1f} us: {mc / ml:.1f} x")
    leaves = [t.clone().requires_grad_(True) for t in block.corr_pyramid]
    ours, theirs = corr_sample1d(leaves, co, r), R.compose_lookup(leaves, co, r)
    bl, bc = _windows([lambda: torch.autograd.grad(ours, leaves, go, retain_graph=True),
                       lambda: torch.autograd.grad(theirs, leaves, go, retain_graph=True)])
    mbl, mbc = statistics.median(bl), statistics.median(bc)
    print(f"  CorrBlock1D lookup backward {mbl * 1e3:.1f} us, composition {mbc * 1e3:.1f} us: {mbc / mbl:.1f} x")
    assert ml <= mc, (tl, tc)
    assert mbl <= mbc, (bl, bc)
