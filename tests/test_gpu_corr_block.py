"""CorrSample / CorrBlock on the GPU (csrc/corr_sample.hip through libflownet2_hip_sample.so, corr_sample_cuda and the Python layer;
include/preview/flownet2_hip_sample.h).

1. forward and backward lie per element within the header's bound of the float64 reference (tests/corr_sample_ref.py), no element
   left out, over ragged pyramids, L = 1 and L = 8, r in {0, 1, 4, 8} and every coordinate family; and, on the first and last
   pixels, at a level whose cell indices pass 2^31;
2. outputs are fully written: pre-filled with NaN they come back free of NaN, the gradient has the bits of +0 outside the G x G box,
   pixels without taps give +0 everywhere;
3. the bits repeat from run to run and on a side stream; under torch.use_deterministic_algorithms(True) nothing is raised or warned;
4. CorrBlock against the float64 composition on the CPU by the rule of tests/pipelines_ref.py (output and both feature gradients);
5. pipelines_ref.mini_raft with CorrBlock as its correlation block, by the same rule;
6. the eager node, the static forward / backward, torch.ops.fn2.corr_sample and a torch.compile'd call give the same bits;
7. both entry points captured raw into a hipGraph, by the procedure of tests/test_gpu_capi_graph.py;
8. forward and backward are not slower than the composition's lookup on the same pyramid (the ratios are printed).

Every output sits inside a larger allocation filled with a sentinel that must be untouched afterwards.
"""
import statistics
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_lookup_ref as RL
import corr_sample_ref as RS
import pipelines_ref as P
from test_gpu_corr_lookup import _guarded, _untouched, _windows

pytestmark = pytest.mark.gpu

RAGGED = ((13, 19), (6, 9), (3, 4), (1, 2))      # down to one row
ONE = ((13, 19),)
EIGHT = ((1, 1),) * 8
# (H, W), the levels, r, coordinate family, pointer offset in elements
CASES = [
    ((5, 67), RAGGED, 4, "a", 0), ((5, 67), RAGGED, 1, "b", 1), ((5, 67), RAGGED, 0, "c", 0), ((5, 67), RAGGED, 8, "g", 0),
    ((5, 67), ONE, 4, "e2", 1), ((5, 67), EIGHT, 1, "c", 0), ((5, 67), ONE, 1, "d", 0),
    ((1, 1), RAGGED, 1, "e2", 0), ((1, 1), EIGHT, 8, "b", 0), ((1, 1), ONE, 4, "a", 1),
    ((4, 64), RAGGED, 4, "d", 0), ((4, 64), ONE, 0, "g", 0), ((4, 64), EIGHT, 4, "e2", 1), ((4, 64), RAGGED, 8, "c", 0),
    ((4, 64), RAGGED, 1, "a", 0), ((4, 64), RAGGED, 4, "g", 1), ((4, 64), RAGGED, 0, "b", 0),
]
assert {c[3] for c in CASES} == set(RS.FAMILIES) and {c[2] for c in CASES} == {0, 1, 4, 8}
WORST = {}


def _case_id(c):
    return "%dx%d-L%d-%dx%d-r%d-%s-off%d" % (*c[0], len(c[1]), *c[1][0], c[2], c[3], c[4])


def _normal(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def _inputs(B, H, W, shapes, r, fam, seed):
    levels = [_normal((B * H * W, 1) + tuple(s), seed + 10 * l) for l, s in enumerate(shapes)]
    co = RS.coords(fam, B, H, W, *shapes[0], r, seed)
    go = _normal((B, len(shapes) * (2 * r + 1) ** 2, H, W), seed + 5)
    return levels, co, go


def _fwd(levels, co, r, off=0, what="forward"):
    import fn2_capi
    B, _, H, W = co.shape
    out, whole = _guarded((B, len(levels) * (2 * r + 1) ** 2, H, W), co.device, off)
    fn2_capi.corr_sample_forward(levels, co, r, out=out)
    _untouched(whole, out, what)
    assert not torch.isnan(out).any(), f"{what}: elements left unwritten"
    return out


def _bwd(levels, co, go, r, off=0, what="backward"):
    import fn2_capi
    held = [_guarded(t.shape, co.device, off) for t in levels]
    fn2_capi.corr_sample_backward(levels, co, go, r, out=[g for g, _ in held])
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
    err, delta = np.abs(got.detach().cpu().numpy().astype(np.float64).reshape(exact.shape) - exact), RS.bound(S)
    ratio = float((err / delta).max())
    assert (err <= delta).all(), f"{what}: {ratio:.3g} x the bound"
    return ratio


# ------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_within_the_headers_bound_and_fully_written(dev, case):
    (H, W), shapes, r, fam, off = case
    B, what = 2, _case_id(case)
    levels, co, go = _inputs(B, H, W, shapes, r, fam, seed=3 * r + H + len(shapes))
    exact, S = RS.forward([t.numpy() for t in levels], co.numpy(), r)
    ref = RS.backward(shapes, co.numpy(), go.numpy(), r)
    lv, cod, god = [t.to(dev) for t in levels], co.to(dev), go.to(dev)
    out = _fwd(lv, cod, r, off, what)
    grads = _bwd(lv, cod, god, r, off, what)
    ratios = [_ratio(out, exact, S, what + " forward")] + [_ratio(g, e, Sg, f"{what} gradient of level {l}")
                                                          for l, (g, (e, Sg, _)) in enumerate(zip(grads, ref))]
    WORST[fam] = max(WORST.get(fam, 0.0), *ratios)
    print(f"  {what}: error / bound forward {ratios[0]:.3f}, backward {max(ratios[1:]):.3f}; family {fam} so far {WORST[fam]:.3f}")
    # exactly +0 where the reference has no term: outside the G x G box, outside the level's reach, pixels without taps
    assert bool((_bits(out).cpu()[torch.from_numpy(S == 0)] == 0).all()), what + ": forward not +0 where no term arrives"
    for l, (g, (_, _, n)) in enumerate(zip(grads, ref)):
        assert bool((_bits(g).cpu().reshape(n.shape)[torch.from_numpy(n == 0)] == 0).all()), f"{what}: level {l} not +0 outside the box"
    ok = torch.from_numpy(RL.decode(co.numpy())[4])
    if fam == "g":
        assert not bool(ok.all())
    if fam in ("d", "g"):
        gone = ~ok if fam == "g" else torch.ones_like(ok)
        if fam == "d":
            assert bool((S == 0).all())
        assert bool((_bits(out).cpu().permute(0, 2, 3, 1)[gone] == 0).all()), what + ": a pixel without taps is not +0"
        for g in grads:
            assert bool((_bits(g).cpu().reshape((B, H, W, -1))[gone] == 0).all()), what + ": a gradient slice without taps is not +0"
    else:
        assert bool(ok.all())


def test_cell_indices_past_2_to_31(dev):
    """One level of 1024 x 1024 cells under 48 x 48 query pixels: 2304 * 2^20 cells, so the slices of the pixels from 2048 on start
    past cell 2^31 (slice bases are 64-bit).  The first and the last 8 pixels are held to the reference and the bound, forward and
    backward; the whole gradient comes back free of NaN inside intact guards."""
    (H, W), (H2, W2), r, n = (48, 48), (1024, 1024), 1, 8
    P_ = H * W
    assert (P_ - n) * H2 * W2 >= 2 ** 31
    cells = ((torch.arange(H2 * W2, device=dev) % 251) - 125).float().view(1, 1, H2, W2) / 64
    level = cells + (torch.arange(P_, device=dev) % 13).float().view(P_, 1, 1, 1)
    co = RS.coords("a", 1, H, W, H2, W2, r, seed=5)
    go = _normal((1, (2 * r + 1) ** 2, H, W), 6)
    cod, god = co.to(dev), go.to(dev)
    out = _fwd([level], cod, r, what="large forward")
    grad, = _bwd([level], cod, god, r, what="large backward")
    for sel in (slice(0, n), slice(P_ - n, P_)):
        sub_co = co.reshape(1, 2, P_)[:, :, sel].reshape(1, 2, 1, n).numpy()
        sub_go = go.reshape(1, -1, P_)[:, :, sel].reshape(1, -1, 1, n).numpy()
        exact, S = RS.forward([level[sel].cpu().numpy()], sub_co, r)
        _ratio(out.reshape(1, -1, P_)[:, :, sel], exact, S, f"large forward, pixels {sel}")
        (e, Sg, cnt), = RS.backward([(H2, W2)], sub_co, sub_go, r)
        _ratio(grad[sel], e, Sg, f"large backward, pixels {sel}")
        assert (cnt > 0).any() and bool((_bits(grad[sel]).cpu().reshape(cnt.shape)[torch.from_numpy(cnt == 0)] == 0).all())


# ------------------------------------------------------------------ 3
def test_bits_repeat_and_deterministic_mode_is_silent(dev):
    from networks.correlation_package import corr_sample
    (H, W), shapes, r = (5, 67), RAGGED, 4
    levels, co, go = _inputs(2, H, W, shapes, r, "a", seed=11)
    lv, cod, god = [t.to(dev) for t in levels], co.to(dev), go.to(dev)
    out, grads = _fwd(lv, cod, r), _bwd(lv, cod, god, r)
    _same_bits(_fwd(lv, cod, r), out, "second forward")
    for g, w in zip(_bwd(lv, cod, god, r), grads):
        _same_bits(g, w, "second backward")
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
            o = corr_sample(leaves, cod, r)
            o.backward(god)
    finally:
        torch.use_deterministic_algorithms(False)
    assert not caught, [str(w.message) for w in caught]
    _same_bits(o.detach(), out, "deterministic mode, forward")
    for t, w in zip(leaves, grads):
        _same_bits(t.grad, w, "deterministic mode, backward")


# ------------------------------------------------------------------ 4
def test_corr_block_against_the_float64_composition(dev):
    from networks.correlation_package import CorrBlock
    B, C, H, W, L, r = 2, 16, 13, 19, 3, 3
    f1, f2 = _normal((B, C, H, W), 1), _normal((B, C, H, W), 2)
    co = RS.coords("a", B, H, W, H, W, r, seed=3)
    go = _normal((B, L * (2 * r + 1) ** 2, H, W), 4)

    def composed(dtype):
        a, b = f1.clone().to(dtype).requires_grad_(True), f2.clone().to(dtype).requires_grad_(True)
        out = RL.compose(a, b, co.to(dtype), r, float(C) ** -0.5, num_levels=L)
        out.backward(go.to(dtype))
        return {"out": out.detach(), "fmap1.grad": a.grad, "fmap2.grad": b.grad}

    o64, o32 = composed(torch.float64), composed(torch.float32)
    a, b = f1.to(dev).requires_grad_(True), f2.to(dev).requires_grad_(True)
    block = CorrBlock(a, b, num_levels=L, radius=r)
    assert [tuple(t.shape) for t in block.corr_pyramid] == [(B * H * W, 1, 13, 19), (B * H * W, 1, 6, 9), (B * H * W, 1, 3, 4)]
    out = block(co.to(dev))
    assert out.shape == (B, L * (2 * r + 1) ** 2, H, W) and out.dtype == torch.float32 and out.is_contiguous()
    out.backward(go.to(dev))
    misses = P.rule_misses({"out": out.detach(), "fmap1.grad": a.grad, "fmap2.grad": b.grad}, o32, o64, "CorrBlock ")
    assert not misses, misses
    assert float(o64["out"].abs().max()) > 0.1 and float(o64["fmap2.grad"].abs().max()) > 0.1


# ------------------------------------------------------------------ 5
def test_mini_raft_with_corr_block(dev):
    from networks.correlation_package import CorrBlock
    from test_gpu_pipelines import by_the_rule, reference
    inp, o64, o32 = reference("raft", 0, dev)
    hip = P.hip_layers()
    layers = types.SimpleNamespace(**{**vars(hip), "corr_block": lambda f1, f2, L, r: CorrBlock(f1, f2, num_levels=L, radius=r)})
    t = P._cast(inp, torch.float32, dev)
    got = P.mini_raft(layers, t)
    by_the_rule(got, o32, o64, "mini-RAFT with CorrBlock")
    before = torch.backends.cudnn.deterministic
    try:   # no atomics are left in the recipe: with the backend's deterministic convolutions every tensor repeats its bits
        torch.backends.cudnn.deterministic = True
        first, again = P.mini_raft(layers, t), P.mini_raft(layers, t)
    finally:
        torch.backends.cudnn.deterministic = before
    differ = [k for k in first if not torch.equal(again[k], first[k])]
    assert not differ, f"second run: {differ} do not repeat their bits"


# ------------------------------------------------------------------ 6
def test_every_door_gives_the_same_bits(dev):
    import torch._dynamo

    import corr_sample_cuda
    from networks.correlation_package import CorrSample, corr_sample
    from networks.correlation_package.corr_block import CorrSampleFunction
    (H, W), shapes, r = (5, 67), RAGGED, 4
    levels, co, go = _inputs(2, H, W, shapes, r, "a", seed=21)
    lv, cod, god = [t.to(dev) for t in levels], co.to(dev), go.to(dev)
    want, wgrads = _fwd(lv, cod, r), _bwd(lv, cod, god, r)
    _same_bits(corr_sample_cuda.forward_alloc(lv, cod, r), want, "forward_alloc")
    for g, w in zip(corr_sample_cuda.backward_alloc(lv, cod, god, r), wgrads):
        _same_bits(g, w, "backward_alloc")

    def static(p, c):      # torch's own Function.apply: it drives the static forward / backward
        return super(CorrSampleFunction, CorrSampleFunction).apply(c, r, *p)

    torch._dynamo.reset()
    doors = (("corr_sample_cuda.apply", lambda p, c: corr_sample_cuda.apply(p, c, r)), ("corr_sample", lambda p, c: corr_sample(p, c, r)),
             ("CorrSample", CorrSample(r)), ("static forward / backward", static),
             ("torch.ops.fn2.corr_sample", lambda p, c: torch.ops.fn2.corr_sample(p, c, r)),
             ("torch.compile", torch.compile(lambda p, c: corr_sample(p, c, r), backend="aot_eager", fullgraph=True)))
    for name, fn in doors:
        leaves = [t.clone().requires_grad_(True) for t in lv]
        out = fn(leaves, cod)
        _same_bits(out.detach(), want, name)
        out.backward(god)
        for t, w in zip(leaves, wgrads):
            _same_bits(t.grad, w, name + " backward")
    with pytest.raises(RuntimeError, match="detach"):
        corr_sample([t.clone().requires_grad_(True) for t in lv], cod.clone().requires_grad_(True), r)
    with pytest.raises(RuntimeError, match="radius"):
        corr_sample_cuda.forward_alloc(lv, cod, 9)
    with pytest.raises(RuntimeError, match="float32"):
        corr_sample_cuda.forward_alloc([t.half() for t in lv], cod, r)
    # non-contiguous levels and coords
    nc = [t.transpose(2, 3).contiguous().transpose(2, 3) for t in lv[:2]] + lv[2:]
    cnc = cod.transpose(2, 3).contiguous().transpose(2, 3)
    assert not nc[0].is_contiguous() and not cnc.is_contiguous()
    _same_bits(corr_sample(nc, cnc, r), want, "non-contiguous inputs")


# ------------------------------------------------------------------ 7
def _graph_cases():
    import capi_graph_cases as G
    import fn2_capi
    B, (H, W), shapes, r = 2, (5, 19), RAGGED, 3
    names = ["level%d" % l for l in range(len(shapes))]
    oshape = (B, len(shapes) * (2 * r + 1) ** 2, H, W)

    def inputs(seed, gout=False):
        levels, co, go = _inputs(B, H, W, shapes, r, "a", seed=100 + seed)
        d = {"coords": co}
        if gout:
            d["grad_out"] = go
        else:
            d.update(zip(names, levels))
        return d

    fwd = G.Case("fn2p_corr_sample_forward", ["fn2p_corr_sample_forward"], inputs, {"out": G.Out(oshape, torch.float32)},
                 lambda T: [G.raised(fn2_capi.corr_sample_forward([T[n] for n in names], T["coords"], r, out=T["out"]))])
    bwd = G.Case("fn2p_corr_sample_backward", ["fn2p_corr_sample_backward"], lambda seed: inputs(seed, gout=True),
                 {"grad_" + n: G.Out((B * H * W, 1) + s, torch.float32) for n, s in zip(names, shapes)},
                 lambda T: [G.raised(fn2_capi.corr_sample_backward([T["grad_" + n] for n in names], T["coords"], T["grad_out"], r,
                                                                   out=[T["grad_" + n] for n in names]))])
    return [fwd, bwd]


@pytest.mark.parametrize("which", [0, 1], ids=["fn2p_corr_sample_forward", "fn2p_corr_sample_backward"])
def test_entry_point_replays_from_a_hip_graph(dev, which):
    import capi_graph_cases as G
    from test_gpu_capi_graph import test_entry_point_replays_from_a_hip_graph as procedure
    case = _graph_cases()[which]
    assert case.id not in [c.id for c in G.CASES]       # built locally: that table is held to include/*.h
    procedure(dev, case)


# ------------------------------------------------------------------ 8
def _composition_lookup(pyramid, coords, r):
    """RAFT's CorrBlock.__call__ on a prebuilt pyramid: grid_sample per level, cat, permute."""
    B, _, H, W = coords.shape
    D = 2 * r + 1
    d = torch.linspace(-r, r, D, dtype=coords.dtype, device=coords.device)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, D, D, 2)
    centroid = coords.permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
    outs = []
    for lvl, corr in enumerate(pyramid):
        h2, w2 = corr.shape[-2:]
        xy = centroid / 2 ** lvl + delta
        grid = torch.stack((2 * xy[..., 0] / (w2 - 1) - 1, 2 * xy[..., 1] / (h2 - 1) - 1), dim=-1)
        outs.append(F.grid_sample(corr, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(B, H, W, D * D))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def test_not_slower_than_the_composition(dev):
    """2 x 64 x 48 x 64, L = 4, r = 4, smooth coordinates, medians over 5 alternating windows of 10 calls.  Only "not slower" is
    asserted, forward and backward each against the composition's on the same pyramid; the ratios are printed (DESIGN.md 4.18 and
    profiles/corr_block_micro.json record the bench script's)."""
    from networks.correlation_package import CorrBlock, corr_sample
    B, C, H, W, L, r = 2, 64, 48, 64, 4, 4
    block = CorrBlock(_normal((B, C, H, W), 1).to(dev), _normal((B, C, H, W), 2).to(dev), num_levels=L, radius=r)
    co = RS.coords("a", B, H, W, H, W, r, seed=4).to(dev)
    go = _normal((B, L * (2 * r + 1) ** 2, H, W), 5).to(dev)
    with torch.no_grad():
        ref, out = _composition_lookup(block.corr_pyramid, co, r), block(co)
        assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max())       # the same function; tests 1 - 5 pin the precision
        tl, tc = _windows([lambda: block(co), lambda: _composition_lookup(block.corr_pyramid, co, r)])
    ml, mc = statistics.median(tl), statistics.median(tc)
    print(f"  CorrBlock lookup forward {ml * 1e3:.1f} us, composition {mc * 1e3:.1f} us: {mc / ml:.1f} x")
    leaves = [t.clone().requires_grad_(True) for t in block.corr_pyramid]
    ours, theirs = corr_sample(leaves, co, r), _composition_lookup(leaves, co, r)
    bl, bc = _windows([lambda: torch.autograd.grad(ours, leaves, go, retain_graph=True),
                       lambda: torch.autograd.grad(theirs, leaves, go, retain_graph=True)])
    mbl, mbc = statistics.median(bl), statistics.median(bc)
    print(f"  CorrBlock lookup backward {mbl * 1e3:.1f} us, composition {mbc * 1e3:.1f} us: {mbc / mbl:.1f} x")
    assert ml <= mc, (tl, tc)
    assert mbl <= mbc, (bl, bc)
