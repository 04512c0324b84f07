"""ForwardWarp on the GPU (include/flownet2_hip_splat.h): the forward of every variant -- general, tiled, auto and the
deterministic entry point -- per cell against the float64 reference inside the header's bound; the exact cases; the validity
edges; the deterministic contract bit for bit; both gradients against their bounds; autograd, the module, ``softsplat`` and
``range_map``.

Every output of a C-ABI call is pre-filled with NaN inside a sentinel-filled allocation that must be untouched afterwards: the
forward has to clear its output itself.

Shapes (B, C, H, W): (1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 17, 67), (2, 5, 33, 130) -- one pixel, less than a wave, ragged against
the FN2S_TILE_H x FN2S_TILE_W = 16 x 64 tile in both directions, and several tiles in both directions with C = 5 against the
channel group of 2.  Flow families (forward_warp_ref.flow_family): smooth, random, converge, zero, shift; each test asserts on
its own input that the family still exercises its branch.  Inputs: standard normal there; at the two larger shapes also
forward_warp_ref.input_family's graded, cancelling, subnormal and huge planes, each under the flows it is meant for.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import forward_warp_ref as RS
import fn2_capi

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 64
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 2, 17, 67), (2, 5, 33, 130)]
LARGE = SHAPES[2:]
FAMILIES = ["smooth", "random", "converge", "zero", "shift"]
VARIANTS = ["general", "tiled", "auto", "det"]
RATIOS = {}   # (quantity, variant or family) -> largest error / bound seen, printed by the last test
U23, SUB = RS.U23, RS.SUB


# ------------------------------------------------------------------ helpers
def _guarded(shape, dev):
    n = int(np.prod(shape))
    whole = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = whole[GUARD:GUARD + n].view(shape)
    view.fill_(float("nan"))
    return view, whole


def _untouched(whole, view, what, nan_ok=False):
    n, lo = view.numel(), view.storage_offset()
    assert bool((whole[:lo] == SENTINEL).all()) and bool((whole[lo + n:] == SENTINEL).all()), f"{what}: wrote outside its output"
    assert nan_ok or not bool(torch.isnan(view).any()), f"{what}: left or produced NaN"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what):
    if isinstance(want, np.ndarray):
        want = torch.tensor(want, device=got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = _bits(got) != _bits(want)
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ; first at flat index {i}: "
                             f"{float(got.flatten()[i])!r} vs {float(want.flatten()[i])!r}")


def _within(got, ref, bound, key, what):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref)
    ratio = float((err / bound).max())
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{what}: largest error / bound {ratio:.3f}")
    if ratio > 1.0:
        i = np.unravel_index(np.argmax(err / bound), err.shape)
        raise AssertionError(f"{what}: error {err[i]:.3e} > bound {bound[i]:.3e} at {i} (ratio {ratio:.3f})")


@lru_cache(maxsize=None)
def _case(shape, family):
    """Inputs and every reference of one (shape, family), computed once and shared; the arrays are read-only."""
    B, C, H, W = shape
    rng = np.random.default_rng(1000 * H + 10 * W + FAMILIES.index(family))
    inp = rng.standard_normal(shape).astype(np.float32)
    go = rng.standard_normal(shape).astype(np.float32)
    flow = RS.flow_family(family, B, H, W)
    out, S, n = RS.forward(inp, flow)
    (gi, Si), (gf, Sf) = RS.backward(inp, flow, go)
    case = dict(inp=inp, go=go, flow=flow, out=out, S=S, n=n, bound=RS.forward_bound(S, n), fixed=RS.forward_fixed(inp, flow), gi=gi, Si=Si,
                gf=gf, Sf=Sf, share=RS.inside_share(flow))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _assert_family(shape, family, c):
    """The condition that keeps a family on its branch, asserted on the test's own input."""
    B, C, H, W = shape
    if family == "smooth" and shape in LARGE:
        assert c["share"] >= 0.8 and (c["n"] >= 2).mean() >= 0.8, (c["share"], (c["n"] >= 2).mean())
    if family == "random" and shape in LARGE:
        assert 0.05 <= c["share"] <= 0.30, c["share"]
    if family == "converge":
        assert c["n"].max() == H * W
    if family == "zero":
        assert c["n"].max() == 1
    if family == "shift":
        assert c["n"].max() == (1 if H > 2 and W > 3 else 0)     # one term per cell; nothing lands in an image of one pixel


def _dev(c, dev, *names):
    return [torch.tensor(c[k], device=dev) for k in names]


def _forward(variant, x, fl):
    """One C-ABI forward into a guarded output."""
    out, whole = _guarded(x.shape, x.device)
    if variant == "det":
        fn2_capi.forward_warp_forward_det(x, fl, out=out)
    else:
        fn2_capi.forward_warp_forward(x, fl, {"general": fn2_capi.FN2S_GENERAL, "tiled": fn2_capi.FN2S_TILED, "auto": fn2_capi.FN2S_AUTO}[variant],
                                      out=out)
    torch.cuda.synchronize()
    return out, whole


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ 1. forward against the bound
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_within_the_bound(dev, shape, family):
    """|out - ref| <= (n + 2) 2^-23 sum |w v| + (n + 2) 2^-149 per cell, for every variant; a cell nothing lands on is +0."""
    c = _case(shape, family)
    _assert_family(shape, family, c)
    x, fl = _dev(c, dev, "inp", "flow")
    empty = torch.from_numpy(c["S"] == 0).to(dev)
    for variant in VARIANTS:
        out, whole = _forward(variant, x, fl)
        _untouched(whole, out, f"{variant} {shape} {family}")
        _within(out, c["out"], c["bound"], ("forward", variant), f"forward {variant} {shape} {family}")
        assert bool((_bits(out)[empty] == 0).all()), f"{variant}: a cell without contributions is not +0"


# ------------------------------------------------------------------ 2. exact cases
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_zero_flow_and_integer_shift_are_exact(dev, shape):
    B, C, H, W = shape
    cz, cs = _case(shape, "zero"), _case(shape, "shift")
    x, = _dev(cz, dev, "inp")
    xs, fls = _dev(cs, dev, "inp", "flow")
    want = torch.zeros_like(xs)
    if H > 2 and W > 3:
        want[:, :, :H - 2, 3:] = xs[:, :, 2:, :W - 3]      # (3, -2): column x to x + 3, row y to y - 2
    results = {}
    for variant in VARIANTS:
        out, whole = _forward(variant, x, torch.zeros(B, 2, H, W, device=dev))
        _untouched(whole, out, f"{variant} zero flow")
        _same_bits(out, x, f"{variant}: zero flow is not the identity")
        out, whole = _forward(variant, xs, fls)
        _untouched(whole, out, f"{variant} shift")
        _same_bits(out, want, f"{variant}: the integer shift is not a shift")
        results[variant] = out
    _same_bits(results["general"], results["tiled"], "general and tiled differ on the integer shift")
    # -0 flows are zero flows too
    out, _ = _forward("tiled", x, -torch.zeros(B, 2, H, W, device=dev))
    _same_bits(out, x, "tiled: a flow of -0 is not the identity")


# ------------------------------------------------------------------ 3. validity edges
def _edge_case():
    """2 x 3 x 5 x 7: the nine edge values as fx of column-0 pixels and as fy of row-0 pixels (coordinate 0, so the flow is the
    position itself); a smooth flow elsewhere.  Returns inputs, the pixels and whether each must be valid."""
    f32 = np.float32
    rng = np.random.default_rng(7)
    B, C, H, W = 2, 3, 5, 7
    inp = rng.standard_normal((B, C, H, W)).astype(f32)
    go = rng.standard_normal((B, C, H, W)).astype(f32)
    flow = (0.75 * rng.standard_normal((B, 2, H, W))).astype(f32)

    def values(n):
        return [f32(-1), f32(n), np.nextafter(f32(n), f32(-np.inf)), np.nextafter(f32(-1), f32(np.inf)), f32(np.nan), f32(np.inf),
                f32(-np.inf), f32(1e30), f32(-1e30)]

    valid = [False, False, True, True, False, False, False, False, False]
    pixels = []
    xpix = [(0, y, 0) for y in range(5)] + [(1, y, 0) for y in range(1, 5)]
    ypix = [(0, 0, x) for x in range(1, 7)] + [(1, 0, x) for x in range(1, 4)]
    for (b, y, x), v, ok in zip(xpix, values(W), valid):
        flow[b, 0, y, x], flow[b, 1, y, x] = v, 0.25
        pixels.append((b, y, x, ok))
    for (b, y, x), v, ok in zip(ypix, values(H), valid):
        flow[b, 1, y, x], flow[b, 0, y, x] = v, -0.25
        pixels.append((b, y, x, ok))
    return inp, go, flow, pixels


def test_validity_edges(dev):
    inp, go, flow, pixels = _edge_case()
    t = RS.taps(flow)
    for b, y, x, ok in pixels:
        assert bool(t["valid"][b, y, x]) == ok, (b, y, x)
    assert len(pixels) == 18 and sum(ok for *_, ok in pixels) == 4
    ref, S, n = RS.forward(inp, flow)
    bound = RS.forward_bound(S, n)
    x, fl, g = (torch.from_numpy(a).to(dev) for a in (inp, flow, go))
    for variant in VARIANTS:
        out, whole = _forward(variant, x, fl)
        _untouched(whole, out, f"{variant} edges")
        _within(out, ref, bound, ("forward", variant), f"forward {variant} validity edges")
    _same_bits(_forward("det", x, fl)[0], RS.forward_fixed(inp, flow), "det at the validity edges")
    gi, gf = fn2_capi.forward_warp_backward(x, fl, g)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(gi).any()) and not bool(torch.isnan(gf).any())
    for b, y, xx, ok in pixels:
        if not ok:
            assert bool((gi[b, :, y, xx] == 0).all()) and bool((gf[b, :, y, xx] == 0).all()), (b, y, xx)
        else:
            assert bool((gi[b, :, y, xx] != 0).any()), (b, y, xx)
    m = RS.header_macros()
    (rgi, Si), (rgf, Sf) = RS.backward(inp, flow, go)
    _within(gi, rgi, m["FN2S_K_I"] * (U23 * Si + SUB), ("grad_input", "edges"), "grad_input validity edges")
    _within(gf, rgf, (3 + m["FN2S_K_F"]) * (U23 * Sf + SUB), ("grad_flow", "edges"), "grad_flow validity edges")


# ------------------------------------------------------------------ 4. deterministic forward
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_deterministic_forward_is_the_fixed_point_contract(dev, shape, family):
    c = _case(shape, family)
    x, fl = _dev(c, dev, "inp", "flow")
    first, whole = _forward("det", x, fl)
    _untouched(whole, first, f"det {shape} {family}")
    _same_bits(first, c["fixed"], f"det {shape} {family}: not the fixed-point result")
    _same_bits(_forward("det", x, fl)[0], first, "det: two calls differ")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other, whole = _guarded(x.shape, dev)
        fn2_capi.forward_warp_forward_det(x, fl, out=other)
    side.synchronize()
    _untouched(whole, other, "det on a side stream")
    _same_bits(other, first, "det: the side stream's result differs")


def test_deterministic_forward_broken_and_zero_planes(dev):
    shape = SHAPES[1]
    c = _case(shape, "smooth")
    bad = c["inp"].copy()
    bad[0, 1, 2, 3] = np.inf
    bad[1, 2, 0, 0] = np.nan
    bad[1, 0] = 0.0
    bad[1, 0, 1, 1] = -0.0
    x, fl = torch.from_numpy(bad).to(dev), torch.tensor(c["flow"], device=dev)
    out, whole = _forward("det", x, fl)
    _untouched(whole, out, "det with broken planes", nan_ok=True)
    want = RS.forward_fixed(bad, c["flow"])
    assert np.isnan(want[0, 1]).all() and np.isnan(want[1, 2]).all() and (want[1, 0] == 0).all()
    got = out.cpu().numpy()
    assert np.isnan(got[0, 1]).all() and np.isnan(got[1, 2]).all()
    assert (got[1, 0].view(np.uint32) == 0).all(), "an all-zero plane is not +0 everywhere"
    for b, ch in ((0, 0), (0, 2), (1, 1)):
        assert (got[b, ch].view(np.uint32) == c["fixed"][b, ch].view(np.uint32)).all(), (b, ch)


def test_module_takes_the_deterministic_path_under_the_flag(dev):
    from networks.splat_package import ForwardWarp
    shape = SHAPES[3]
    c = _case(shape, "smooth")
    x, fl = _dev(c, dev, "inp", "flow")
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        for warn_only in (False, True):
            torch.use_deterministic_algorithms(True, warn_only=warn_only)
            _same_bits(ForwardWarp()(x, fl), c["fixed"], f"module under the deterministic flag (warn_only={warn_only})")
        torch.use_deterministic_algorithms(False)
        _within(ForwardWarp()(x, fl), c["out"], c["bound"], ("forward", "module"), "module without the flag")
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


# ------------------------------------------------------------------ 5. backward against the bounds
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_within_the_bounds(dev, shape, family):
    """grad_input within K_I 2^-23 sum |w gO|, grad_flow within (C + K_F) 2^-23 sum_c |input_c| (...), the constants read from
    the header; the same bits from run to run, and from the calls that want one gradient only."""
    c = _case(shape, family)
    m = RS.header_macros()
    KI, KF = m["FN2S_K_I"], m["FN2S_K_F"]
    assert (KI, KF) == (6, 4)
    x, fl, g = _dev(c, dev, "inp", "flow", "go")
    gi, gf = fn2_capi.forward_warp_backward(x, fl, g)
    torch.cuda.synchronize()
    _within(gi, c["gi"], KI * (U23 * c["Si"] + SUB), ("grad_input", family), f"grad_input {shape} {family}")
    _within(gf, c["gf"], (shape[1] + KF) * (U23 * c["Sf"] + SUB), ("grad_flow", family), f"grad_flow {shape} {family}")
    gi2, gf2 = fn2_capi.forward_warp_backward(x, fl, g)
    _same_bits(gi2, gi, "grad_input: two runs differ")
    _same_bits(gf2, gf, "grad_flow: two runs differ")
    only_i, none = fn2_capi.forward_warp_backward(x, fl, g, want_flow=False)
    assert none is None
    _same_bits(only_i, gi, "grad_input alone differs from the full call")
    none, only_f = fn2_capi.forward_warp_backward(x, fl, g, want_input=False)
    assert none is None
    _same_bits(only_f, gf, "grad_flow alone differs from the full call")



# ------------------------------------------------------------------ 9. hipGraph replay
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
def test_forward_replays_from_a_hip_graph(dev, det):
    """The forward adds into its output (the deterministic one into its workspace), so the clear the entry point enqueues is
    part of the result: captured into a hipGraph it has to clear on EVERY replay.  The module's forward is captured once and
    replayed on three inputs in the captured buffers, the captured output poisoned with NaN before each replay; a clear that
    does not run leaves the NaN (or, in the workspace, the last replay's sums).  Atomic path: inside the forward bound;
    deterministic path: the bits of the fixed-point contract."""
    from networks.splat_package import ForwardWarp
    shape = (2, 3, 17, 67)
    cases = [_case(shape, f) for f in ("smooth", "random", "converge")]
    x, fl = _dev(cases[0], dev, "inp", "flow")
    layer = ForwardWarp()
    try:
        torch.use_deterministic_algorithms(det)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(3):
                layer(x, fl)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            out = layer(x, fl)
    finally:
        torch.use_deterministic_algorithms(False)
    for c in cases[1:] + cases[:1]:
        nx, nfl = _dev(c, dev, "inp", "flow")
        x.copy_(nx)
        fl.copy_(nfl)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert not torch.isnan(out).any(), "the replay left the poison: the output was not cleared"
        if det:
            _same_bits(out, c["fixed"], "deterministic forward replayed from a hipGraph")
        else:
            _within(out, c["out"], c["bound"], ("forward", "graph"), "forward replayed from a hipGraph")
        empty = torch.from_numpy(c["S"] == 0).to(dev)
        assert bool((_bits(out)[empty] == 0).all()), "replayed from a hipGraph: a cell without contributions is not +0"

# ------------------------------------------------------------------ 6. autograd and modules
def test_autograd_is_the_raw_calls(dev):
    from networks.splat_package import ForwardWarp, ForwardWarpFunction
    c = _case(SHAPES[3], "smooth")
    x, fl, g = _dev(c, dev, "inp", "flow", "go")
    gi, gf = fn2_capi.forward_warp_backward(x, fl, g)
    a, f = x.clone().requires_grad_(True), fl.clone().requires_grad_(True)
    out = ForwardWarp()(a, f)
    _within(out, c["out"], c["bound"], ("forward", "module"), "module forward")
    out.backward(g)
    _same_bits(a.grad, gi, "autograd grad_input")
    _same_bits(f.grad, gf, "autograd grad_flow")
    # needs_input_grad: one gradient only
    a = x.clone().requires_grad_(True)
    ForwardWarpFunction.apply(a, fl).backward(g)
    _same_bits(a.grad, gi, "input-only grad_input")
    f = fl.clone().requires_grad_(True)
    ForwardWarpFunction.apply(x, f).backward(g)
    _same_bits(f.grad, gf, "flow-only grad_flow")
    assert not ForwardWarpFunction.apply(x, fl).requires_grad
    # non-contiguous inputs are made contiguous
    xt = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous()
    _within(ForwardWarp()(xt, fl), c["out"], c["bound"], ("forward", "module"), "module forward, strided input")


def test_softsplat_modes_and_range_map(dev):
    from networks.splat_package import ForwardWarpFunction, range_map, softsplat
    import forward_warp_cuda
    shape = SHAPES[3]
    c = _case(shape, "shift")     # at most one term per cell: the atomic sums are exact, so compositions compare bit for bit
    x, fl = _dev(c, dev, "inp", "flow")
    metric = torch.from_numpy(np.random.default_rng(11).standard_normal((shape[0], 1) + shape[2:]).astype(np.float32)).to(dev)
    ones = torch.ones_like(metric)
    S = ForwardWarpFunction.apply
    _same_bits(softsplat(x, fl), S(x, fl), "softsplat sum")
    o = S(torch.cat([x, ones], 1), fl)
    _same_bits(softsplat(x, fl, mode="avg"), o[:, :-1] / (o[:, -1:] + 1e-7), "softsplat avg")
    o = S(torch.cat([x * metric, metric], 1), fl)
    _same_bits(softsplat(x, fl, metric, mode="linear"), o[:, :-1] / (o[:, -1:] + 1e-7), "softsplat linear")
    o = S(torch.cat([x * metric.exp(), metric.exp()], 1), fl)
    _same_bits(softsplat(x, fl, metric, mode="soft"), o[:, :-1] / (o[:, -1:] + 1e-7), "softsplat soft")
    # the average of a constant image is that constant wherever something lands.  The 1e-7 in the denominator costs 1e-7 / range
    # relative, so the flow is the smooth family on a grid of half pixels: every weight is a multiple of 1/4, both splats are
    # exact, a cell that receives anything has range >= 1/4, and the deviation is 4e-7 plus one rounding of the division
    cs = _case(shape, "smooth")
    flh = torch.tensor(np.rint(cs["flow"] * 2) / 2, device=dev)
    const = torch.full(shape, 3.25, device=dev)
    avg, rm = softsplat(const, flh, mode="avg"), range_map(flh)
    assert rm.shape == (shape[0], 1) + shape[2:]
    hit = (rm > 1e-3).expand_as(avg)
    assert float(hit.float().mean()) > 0.8 and float(rm[rm > 1e-3].min()) >= 0.25 and bool((rm == 0).any())
    assert float(((avg - 3.25).abs() / 3.25)[hit].max()) <= 2.0 ** -20
    fls, = _dev(cs, dev, "flow")
    ref1, S1, n1 = RS.forward(np.ones((shape[0], 1) + shape[2:], np.float32), cs["flow"])
    _within(range_map(fls), ref1, RS.forward_bound(S1, n1), ("forward", "module"), "range_map")
    _same_bits(range_map(torch.zeros(2, 2, 9, 70, device=dev)), torch.ones(2, 1, 9, 70, device=dev), "range_map of a zero flow")
    # softsplat is differentiable in input, flow and metric
    a, f, mt = x.clone().requires_grad_(True), fls.clone().requires_grad_(True), metric.clone().requires_grad_(True)
    softsplat(a, f, mt, mode="soft").sum().backward()
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0 for t in (a, f, mt))
    # a non-default stream, the device selected explicitly
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.device(0), torch.cuda.stream(side):
        out = forward_warp_cuda.forward_alloc(*_dev(cs, dev, "inp", "flow"))
    side.synchronize()
    _within(out, cs["out"], cs["bound"], ("forward", "module"), "forward on a side stream, device 0 selected")


# ------------------------------------------------------------------ 10. the input families
NEW_INPUTS = [f for f in RS.INPUT_FAMILIES if f != "normal"]


@lru_cache(maxsize=None)
def _family_case(shape, family, flow_name):
    """One (shape, input family, flow family): inputs and references, computed once and shared; the arrays are read-only.  The
    input family asserts its own condition when it is drawn."""
    B, C, H, W = shape
    inp, go = RS.input_family(family, shape, 1000 * H + 10 * W + 50 + RS.INPUT_FAMILIES.index(family))
    flow = RS.flow_family(flow_name, B, H, W)
    out, S, n = RS.forward(inp, flow)
    case = dict(inp=inp, go=go, flow=flow, out=out, S=S, n=n, bound=RS.forward_bound(S, n), fixed=RS.forward_fixed(inp, flow))
    if family != "huge":      # its gradients overflow
        (case["gi"], case["Si"]), (case["gf"], case["Sf"]) = RS.backward(inp, flow, go)
    for v in case.values():
        v.setflags(write=False)
    return case


@pytest.mark.parametrize("family", NEW_INPUTS)
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "x".join(map(str, s)))
def test_input_families_forward_within_the_bound(dev, shape, family):
    """Graded, cancelling, subnormal and huge inputs under the flows they are meant for: every variant inside the header's
    forward bound per cell -- its floor is (n + 2) 2^-149, so a subnormal sum has to survive the atomics --, a cell nothing lands
    on +0, and the deterministic entry point the bits of the fixed-point contract, for plane maxima from 2^-127 to 2^126."""
    for flow_name in RS.FAMILY_FLOWS[family]:
        c = _family_case(shape, family, flow_name)
        x, fl = _dev(c, dev, "inp", "flow")
        empty = torch.from_numpy(c["S"] == 0).to(dev)
        assert np.isfinite(c["out"]).all() and np.isfinite(c["bound"]).all()
        for variant in VARIANTS:
            what = f"{variant} {shape} {family} {flow_name}"
            out, whole = _forward(variant, x, fl)
            _untouched(whole, out, what)
            _within(out, c["out"], c["bound"], ("forward " + family, variant), "forward " + what)
            assert bool((_bits(out)[empty] == 0).all()), f"{what}: a cell without contributions is not +0"
            if variant == "det":
                _same_bits(out, c["fixed"], f"{what}: not the fixed-point result")


@pytest.mark.parametrize("family", ["graded", "cancel", "subnormal"])
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "x".join(map(str, s)))
def test_input_families_backward_within_the_bounds(dev, shape, family):
    """Both gradients inside the header's bounds on the graded, cancelling and subnormal inputs; two runs give the same bits."""
    m = RS.header_macros()
    KI, KF = m["FN2S_K_I"], m["FN2S_K_F"]
    for flow_name in RS.FAMILY_FLOWS[family]:
        c = _family_case(shape, family, flow_name)
        x, fl, g = _dev(c, dev, "inp", "flow", "go")
        what = f"{shape} {family} {flow_name}"
        gi, gf = fn2_capi.forward_warp_backward(x, fl, g)
        torch.cuda.synchronize()
        _within(gi, c["gi"], KI * (U23 * c["Si"] + SUB), ("grad_input " + family, flow_name), "grad_input " + what)
        _within(gf, c["gf"], (shape[1] + KF) * (U23 * c["Sf"] + SUB), ("grad_flow " + family, flow_name), "grad_flow " + what)
        gi2, gf2 = fn2_capi.forward_warp_backward(x, fl, g)
        _same_bits(gi2, gi, what + " grad_input: two runs differ")
        _same_bits(gf2, gf, what + " grad_flow: two runs differ")


def test_report_largest_ratios():
    """Last: the largest error / bound ratios of this run, for DESIGN 4.13."""
    for key in sorted(RATIOS):
        print("largest error / bound", key, f"{RATIOS[key]:.3f}")
    assert RATIOS and max(RATIOS.values()) <= 1.0
