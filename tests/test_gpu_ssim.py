"""The structural-similarity distance on the GPU (include/staging/flownet2_hip_ssim.h): the forward and both gradients per element
against the float64 reference inside half of the header's bounds and, independently, per tensor inside the rule of DESIGN.md 4.16
made of the float32 composition's own error; the exact facts (the zero ring, the reach of one grad_out pixel -- its k x k window --
the folded corner under reflect, identical images, one gradient asked for alone); repeatable bits; strided and misaligned inputs;
the refusals; autograd through ``SSIMLoss``; raw and module-level graph capture; ``torch.compile``.

Every buffer of a C-ABI call sits inside a sentinel-filled allocation that must be untouched afterwards; outputs are pre-filled
with NaN: the kernels have to write every element of their outputs themselves, and nothing else.

Shapes (N, C, H, W), T = FN2I_TILE_H x FN2I_TILE_W read from the header: (1, 1, 1, 1) and (1, 1, 2, 2), the smallest a border mode
admits; (1, 2, 3, 3), one valid cell at md = 1; (1, 1, 6, 7), smaller than k at md = 3 in zero mode; (2, 3, 5, 7), ragged;
(1, 1, T_H + 1, T_W + 1), ragged last tiles; (2, 3, 2 T_H + md, 2 T_W + 2 md + 1), the backward's halo of 2 md across tile seams;
(1, 4, 16, 64) on the 16-byte row path and (1, 1, 17, 65) one past it.  Each with every md it admits, both borders, and the
families noise, smooth and bytes of tests/ssim_ref.py.

Largest error / bound seen on an MI355X (test_report_largest_ratios prints them): see DESIGN.md 4.20.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import fn2_capi
import pipelines_ref as P
import ssim_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 64          # floats: 256 bytes, so a guarded view starts on 16 bytes
TH, TW = R.TILE_H, R.TILE_W
MDS = (1, 2, 3)
BORDERS = ("zero", "reflect")
FAMILIES = ("noise", "smooth", "bytes")
RATIOS = {}         # (quantity, family) -> largest error / bound seen, printed by the last test
RULE = {}           # quantity -> largest error / rule bound seen


def shapes(md):
    return [(1, 1, 1, 1), (1, 1, 2, 2), (1, 2, 3, 3), (1, 1, 6, 7), (2, 3, 5, 7), (1, 1, TH + 1, TW + 1),
            (2, 3, 2 * TH + md, 2 * TW + 2 * md + 1), (1, 4, 16, 64), (1, 1, 17, 65)]


CASES = [(s, md, b) for md in MDS for s in dict.fromkeys(shapes(md)) for b in BORDERS if R.admits(s, md, b)]
_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))


# ------------------------------------------------------------------ helpers
def _guarded(shape, dev, values=None):
    """A contiguous float32 view inside a sentinel-filled allocation: NaN, or ``values``."""
    n = int(np.prod(shape))
    whole = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = whole[GUARD:GUARD + n].view(shape)
    if values is None:
        view.fill_(float("nan"))
    else:
        view.copy_(values)
    return view, whole


def _untouched(whole, view, what, values=None):
    n, lo = view.numel(), view.storage_offset()
    assert bool((whole[:lo] == SENTINEL).all()) and bool((whole[lo + n:] == SENTINEL).all()), f"{what}: wrote outside its buffer"
    if values is None:
        assert not bool(torch.isnan(view).any()), f"{what}: left or produced NaN"
    else:
        assert torch.equal(_bits(view.cpu()), _bits(values.float())), f"{what}: an input was written"   # (bits: NaN compares unequal)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = _bits(got) != _bits(want)
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ; first at flat index {i}: "
                             f"{float(got.flatten()[i])!r} vs {float(want.flatten()[i])!r}")


def _within_half(got, ref, bound, key, what):
    """err <= bound / 2 per element; where the bound is 0 the value is exactly 0.  Prints the largest err / bound first."""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{what}: largest error / bound {ratio:.4f}")
    assert bool((got[zero] == 0).all()), f"{what}: not exactly 0 where the bound is 0"
    assert ratio <= 0.5, f"{what}: error / bound {ratio:.3f} above a half"


def _rule(got, t32, ref, key, what):
    """max |hip - f64| <= max(8 max |comp32 - f64|, 2^-20 max |f64|), per tensor."""
    err = float((got.detach().cpu().double() - ref).abs().max()) if ref.numel() else 0.0
    bound = P.rule_bound(t32, ref) if ref.numel() else 0.0
    print(f"{what}: error {err:.3g}, rule bound {bound:.3g}")
    if bound > 0:
        RULE[key] = max(RULE.get(key, 0.0), err / bound)
    assert err <= bound, f"{what}: error {err:.3g} above the rule's bound {bound:.3g}"


@lru_cache(maxsize=None)
def _case(shape, md, border, family):
    """Inputs, the float64 reference with its bounds and the float32 composition of one case, computed once and shared."""
    x, y, go = R.inputs(shape, family)
    c1, c2 = R.constants(family)
    ref = R.reference(x, y, go, md, c1, c2, border)
    a, b = x.float().requires_grad_(True), y.float().requires_grad_(True)
    o32 = R.compose(a, b, md, c1, c2, border)
    g32 = torch.autograd.grad(o32, (a, b), go.float(), allow_unused=True)
    comp = [o32.detach()] + [torch.zeros_like(a) if g is None else g for g in g32]
    return dict(x=x, y=y, go=go, c1=c1, c2=c2, ref=ref, comp=comp)


def _forward(x, y, md, c1, c2, border, dev):
    (a, wa), (b, wb) = _guarded(x.shape, dev, x), _guarded(x.shape, dev, y)
    out, wo = _guarded(x.shape, dev)
    fn2_capi.ssim_forward(a, b, md, c1, c2, border, out=out)
    torch.cuda.synchronize()
    _untouched(wo, out, "forward")
    _untouched(wa, a, "forward im1", x)
    _untouched(wb, b, "forward im2", y)
    return out


def _backward(x, y, go, md, c1, c2, border, dev, want1=True, want2=True):
    (a, wa), (b, wb), (g, wg) = _guarded(x.shape, dev, x), _guarded(x.shape, dev, y), _guarded(x.shape, dev, go)
    (g1, w1), (g2, w2) = _guarded(x.shape, dev), _guarded(x.shape, dev)
    r1, r2 = fn2_capi.ssim_backward(a, b, g, md, c1, c2, border, want1, want2, grads=(g1, g2))
    torch.cuda.synchronize()
    for want, r, t, w, name in ((want1, r1, g1, w1, "grad1"), (want2, r2, g2, w2, "grad2")):
        if want:
            _untouched(w, t, name)
        else:   # not wanted: not written at all
            assert r is None and bool(torch.isnan(t).all()) and bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all())
    for t, w, v, name in ((a, wa, x, "im1"), (b, wb, y, "im2"), (g, wg, go, "grad_out")):
        _untouched(w, t, "backward " + name, v)
    return g1, g2


# ------------------------------------------------------------------ 1. per element, and the rule
@pytest.mark.parametrize("shape,md,border", CASES, **_ids)
def test_forward_and_backward_within_half_the_bound(dev, shape, md, border):
    for family in FAMILIES:
        c = _case(shape, md, border, family)
        ref, what = c["ref"], f"{family} md {md} {border}"
        assert family == "identical" or ref["margin"] > 4, ref["margin"]
        out = _forward(c["x"], c["y"], md, c["c1"], c["c2"], border, dev)
        g1, g2 = _backward(c["x"], c["y"], c["go"], md, c["c1"], c["c2"], border, dev)
        for name, got, r, bd, t32 in (("out", out, ref["out"], ref["bound"], c["comp"][0]), ("grad1", g1, ref["g1"], ref["bound1"], c["comp"][1]),
                                      ("grad2", g2, ref["g2"], ref["bound2"], c["comp"][2])):
            _within_half(got, r, bd, (name, family), f"{what} {name}")
            _rule(got, t32, r, name, f"{what} {name}")


# ------------------------------------------------------------------ 2. exact facts
@pytest.mark.parametrize("md", MDS)
def test_zero_ring_is_exact_and_sends_no_gradient(dev, md):
    shape = (2, 3, 2 * TH + md, 2 * TW + 2 * md + 1)
    c = _case(shape, md, "zero", "noise")
    ring = (R.valid_mask(shape, md, "zero") == 0).expand(shape)
    out = _forward(c["x"], c["y"], md, c["c1"], c["c2"], "zero", dev).cpu()
    assert bool((_bits(out)[ring] == 0).all())                  # +0, not -0
    go = c["go"].clone()
    g1, g2 = _backward(c["x"], c["y"], go, md, c["c1"], c["c2"], "zero", dev)
    go[ring] = float("nan")                                     # grad_out on the ring is not read as a number
    n1, n2 = _backward(c["x"], c["y"], go, md, c["c1"], c["c2"], "zero", dev)
    _same_bits(n1, g1, "grad1 with NaN on the ring")
    _same_bits(n2, g2, "grad2 with NaN on the ring")
    only = torch.zeros(shape, dtype=torch.float64)
    only[ring] = c["go"][ring]
    z1, z2 = _backward(c["x"], c["y"], only, md, c["c1"], c["c2"], "zero", dev)
    assert bool((z1 == 0).all()) and bool((z2 == 0).all())


@pytest.mark.parametrize("md", MDS)
def test_one_grad_out_pixel_reaches_its_window_and_nothing_else(dev, md):
    """out[p] is a function of the k x k window of p alone, so one grad_out pixel reaches exactly those k^2 pixels of each image --
    every one of them, and nothing else -- in zero mode at an interior pixel.  (The (2 k - 1)^2 pixels within 2 md are what the
    kernel reads for a tile's pixel, not what one window reaches; the float64 reference, held to autograd of the composition by
    tests/test_ssim_host.py, is checked for the same reach here.)"""
    shape, k = (1, 2, 2 * TH + md, 2 * TW + 2 * md + 1), 2 * md + 1
    x, y, _ = R.inputs(shape, "noise")
    py, px = TH, TW                                             # interior, its window across both tile seams
    go = torch.zeros(shape, dtype=torch.float64)
    go[0, 1, py, px] = 1.0
    reach = torch.zeros(shape, dtype=torch.bool)
    reach[0, 1, py - md:py + md + 1, px - md:px + md + 1] = True
    assert int(reach.sum()) == k * k
    ref = R.reference(x, y, go, md, R.C1, R.C2, "zero")
    for g, r in zip(_backward(x, y, go, md, R.C1, R.C2, "zero", dev), (ref["g1"], ref["g2"])):
        g = g.cpu()
        assert bool((r[reach] != 0).all()) and bool((r[~reach] == 0).all())
        assert bool((g[reach] != 0).all()) and bool((g[~reach] == 0).all())


@pytest.mark.parametrize("md", MDS)
def test_reflect_folds_the_corner_gradient(dev, md):
    """grad_out at the four corner pixels alone: the gradient is confined to the 2 md + 1 pixels from each corner and agrees with
    the composition's (float64, autograd through ReflectionPad2d) inside half the bound at every folded position."""
    shape = (1, 1, TH + 1, TW + 1)
    x, y, _ = R.inputs(shape, "noise")
    H, W = shape[2:]
    go = torch.zeros(shape, dtype=torch.float64)
    for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        go[0, 0, cy, cx] = 1.0 + cy / H + cx / W
    ref = R.reference(x, y, go, md, R.C1, R.C2, "reflect")
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    w1, w2 = torch.autograd.grad(R.compose(a, b, md, R.C1, R.C2, "reflect"), (a, b), go)
    g1, g2 = _backward(x, y, go, md, R.C1, R.C2, "reflect", dev)
    near = torch.zeros(shape, dtype=torch.bool)
    for ys in (slice(0, 2 * md + 1), slice(H - 2 * md - 1, H)):
        for xs in (slice(0, 2 * md + 1), slice(W - 2 * md - 1, W)):
            near[0, 0, ys, xs] = True
    for name, got, want, r, bd in (("grad1", g1, w1, ref["g1"], ref["bound1"]), ("grad2", g2, w2, ref["g2"], ref["bound2"])):
        assert float((r - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert float(want[0, 0, 0, 1].abs()) > 0 and bool((got.cpu()[~near] == 0).all())
        _within_half(got, want, bd, (name, "corner"), f"corner md {md} {name}")


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("md", MDS)
def test_identical_images(dev, md, border):
    """The clamp's edge: the distance is at most its bound (in fact +0: S = 1 bit for bit) and both gradients are at most theirs
    in magnitude, whichever side of the clamp rounding falls on."""
    c = _case((2, 3, 2 * TH + md, 2 * TW + 2 * md + 1), md, border, "identical")
    ref = c["ref"]
    assert float(ref["out"].abs().max()) == 0 and float(ref["g1"].abs().max()) < 1e-12
    out = _forward(c["x"], c["y"], md, c["c1"], c["c2"], border, dev).cpu()
    g1, g2 = _backward(c["x"], c["y"], c["go"], md, c["c1"], c["c2"], border, dev)
    assert bool((out.double() <= ref["bound"]).all()) and bool((_bits(out) == 0).all())
    for name, g, bd in (("grad1", g1, ref["bound1"]), ("grad2", g2, ref["bound2"])):
        ratio = float((g.cpu().double().abs()[bd > 0] / bd[bd > 0]).max())
        RATIOS[(name, "identical")] = max(RATIOS.get((name, "identical"), 0.0), ratio)
        assert ratio <= 1.0 and bool((g.cpu()[bd == 0] == 0).all()), (name, ratio)


@pytest.mark.parametrize("border", BORDERS)
def test_one_gradient_alone_has_the_same_bits(dev, border):
    c = _case((2, 3, 5, 7), 2, border, "noise")
    args = (c["x"], c["y"], c["go"], 2, c["c1"], c["c2"], border, dev)
    g1, g2 = _backward(*args)
    a1, _ = _backward(*args, want2=False)
    _, a2 = _backward(*args, want1=False)
    _same_bits(a1, g1, "grad1 alone")
    _same_bits(a2, g2, "grad2 alone")


# ------------------------------------------------------------------ 3. repeatable bits
@pytest.mark.parametrize("border", BORDERS)
def test_runs_and_streams_are_bit_identical(dev, border):
    from networks.ssim_package import ssim_distance
    c = _case((2, 3, 2 * TH + 3, 2 * TW + 7), 3, border, "noise")
    x, y, go = (c[k].float().to(dev) for k in ("x", "y", "go"))

    def run():
        a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        out = ssim_distance(a, b, 3, border=border)
        out.backward(go)
        return out.detach(), a.grad, b.grad

    first = run()
    for i in range(2):
        for got, want, name in zip(run(), first, ("out", "grad1", "grad2")):
            _same_bits(got, want, f"run {i + 2} {name}")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run()
    side.synchronize()
    torch.use_deterministic_algorithms(True)
    try:
        det = run()
    finally:
        torch.use_deterministic_algorithms(False)
    for got, d, want, name in zip(other, det, first, ("out", "grad1", "grad2")):
        _same_bits(got, want, f"side stream {name}")
        _same_bits(d, want, f"deterministic {name}")


# ------------------------------------------------------------------ 4. other input forms, refusals
@pytest.mark.parametrize("border", BORDERS)
def test_strided_and_misaligned_inputs_give_the_contiguous_bits(dev, border):
    """The binding copies what is not contiguous (census_cuda's policy); a contiguous tensor four bytes off a 16-byte boundary takes
    the one-float staging path.  Both give the bits of the aligned contiguous call, forward and backward."""
    from networks.ssim_package import ssim_distance
    shape = (2, 4, 16, 64)
    x, y, go = (t.float().to(dev) for t in R.inputs(shape, "noise"))

    def run(a, b):
        a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
        out = ssim_distance(a, b, 2, border=border)
        out.backward(go)
        return out.detach(), a.grad, b.grad

    want = run(x, y)
    wide = [torch.cat([t, t.flip(3)], 3) for t in (x, y)]
    off = []
    for t in (x, y):
        buf = torch.empty(t.numel() + 1, device=dev)
        buf[1:].copy_(t.flatten())
        off.append(buf[1:].view(shape))
        assert off[-1].data_ptr() % 16 == 4 and off[-1].is_contiguous()
    forms = {"channels-last": [t.contiguous(memory_format=torch.channels_last) for t in (x, y)],
             "a W-slice": [w[..., :shape[3]] for w in wide], "misaligned": off}
    for name, (a, b) in forms.items():
        assert name == "misaligned" or not a.is_contiguous()
        for got, w, q in zip(run(a, b), want, ("out", "grad1", "grad2")):
            _same_bits(got.contiguous(), w, f"{name} {q}")


def test_other_dtypes_and_cpu_tensors_are_refused(dev):
    from networks.ssim_package import ssim_distance
    a = torch.rand(1, 1, 8, 8, device=dev)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(RuntimeError, match=r"im1 must be float32, got .*: convert it with \.float\(\)"):
            ssim_distance(a.to(dt), a.to(dt))
        with pytest.raises(RuntimeError, match=r"im2 must be float32, got .*: convert it with \.float\(\)"):
            ssim_distance(a, a.to(dt))
    with pytest.raises(RuntimeError, match="im2 must be a GPU .HIP. tensor; this extension has no CPU implementation"):
        ssim_distance(a, a.cpu())
    with pytest.raises(RuntimeError, match="im1 must be a GPU"):
        ssim_distance(a.cpu(), a)
    empty = ssim_distance(a[:0], a[:0], border="reflect")
    assert empty.shape == (0, 1, 8, 8) and empty.dtype == torch.float32


# ------------------------------------------------------------------ 5. autograd
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_ssim_loss_matches_its_float64_composition(dev, border, masked):
    from networks.ssim_package import SSIMLoss
    shape, md = (2, 3, 2 * TH + 2, 2 * TW + 5), 2
    x, y, m = R.inputs(shape, "noise", seed=7)
    mask = (m[:, :1] > -0.5).double() if masked else None
    out = {}
    for key, dtype, device in (("hip", torch.float32, dev), ("f32", torch.float32, "cpu"), ("f64", torch.float64, "cpu")):
        a, b = (t.to(device=device, dtype=dtype).requires_grad_(True) for t in (x, y))
        mk = None if mask is None else mask.to(device=device, dtype=dtype)
        loss = SSIMLoss(md, border)(a, b, mk) if key == "hip" else R.compose_loss(a, b, mk, md, border)
        loss.backward()
        out[key] = {"loss": loss.detach(), "im1.grad": a.grad, "im2.grad": b.grad}
    assert float(out["f64"]["loss"]) > 0.01
    assert P.rule_misses(out["hip"], out["f32"], out["f64"], f"SSIMLoss {border} ") == []


def test_second_order_differentiation_raises(dev):
    from networks.ssim_package import ssim_distance
    a, b = (torch.rand(1, 1, 8, 8, device=dev).requires_grad_(True) for _ in range(2))
    go = torch.ones(1, 1, 8, 8, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="SSIMFunction.backward: the backward of this layer is a HIP kernel and not differentiable a second time"):
        torch.autograd.grad(ssim_distance(a, b), a, go, create_graph=True)
    o = torch.ops.fn2.ssim(a, b, 1, 1e-4, 9e-4, 0)
    g, = torch.autograd.grad(o.sum(), a, create_graph=True)
    with pytest.raises(RuntimeError, match="fn2::ssim_backward: the backward of this layer is a HIP kernel and not differentiable a second time"):
        g.sum().backward()


# ------------------------------------------------------------------ 6. graph capture
def _capture(step):
    """The pattern of tests/test_gpu_capi_graph.py: three warm-up runs on a side stream, then the capture."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


@pytest.mark.parametrize("border", BORDERS)
def test_raw_entry_points_replay_from_a_graph(dev, border):
    """Both entry points captured raw (ctypes, torch's capture stream) into one graph; three replays on fresh values into outputs
    poisoned with NaN give the eager call's bits.  include/staging/ is outside the table of tests/capi_graph_cases.py."""
    shape, md = (2, 3, TH + 3, TW + 5), 2
    bufs = {k: _guarded(shape, dev, torch.zeros(shape)) for k in ("x", "y", "go")}
    outs = {k: _guarded(shape, dev) for k in ("out", "g1", "g2")}

    def step():
        fn2_capi.ssim_forward(bufs["x"][0], bufs["y"][0], md, R.C1, R.C2, border, out=outs["out"][0])
        fn2_capi.ssim_backward(bufs["x"][0], bufs["y"][0], bufs["go"][0], md, R.C1, R.C2, border, grads=(outs["g1"][0], outs["g2"][0]))

    graph = _capture(step)
    for seed in (1, 2, 3):
        vals = dict(zip(("x", "y", "go"), R.inputs(shape, "noise", seed=seed)))
        for k, (view, _) in bufs.items():
            view.copy_(vals[k])
        for view, _ in outs.values():
            view.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want_out = _forward(vals["x"], vals["y"], md, R.C1, R.C2, border, dev)
        want = dict(zip(("g1", "g2"), _backward(vals["x"], vals["y"], vals["go"], md, R.C1, R.C2, border, dev)), out=want_out)
        for k, (view, whole) in outs.items():
            _untouched(whole, view, f"replay {seed} {k}")
            assert float(view.abs().max()) > 0
            _same_bits(view, want[k], f"replay {seed} {k}")
    for k, (view, whole) in bufs.items():
        _untouched(whole, view, f"captured input {k}", vals[k])


def test_module_replays_from_a_graph(dev):
    from networks.ssim_package import SSIMLoss
    shape = (2, 3, TH + 3, TW + 5)
    loss_fn = SSIMLoss(md=3, border="reflect")
    a, b = (torch.zeros(shape, device=dev).requires_grad_(True) for _ in range(2))
    res = {}

    def step():
        a.grad = b.grad = None
        loss = loss_fn(a, b)
        res["g1"], res["g2"] = torch.autograd.grad(loss, (a, b))
        res["loss"] = loss.detach()

    with torch.no_grad():
        for t, v in zip((a, b), R.inputs(shape, "noise", seed=9)):
            t.copy_(v)
    graph = _capture(step)
    for seed in (1, 2, 3):
        x, y, _ = R.inputs(shape, "noise", seed=seed)
        with torch.no_grad():
            a.copy_(x)
            b.copy_(y)
        for t in res.values():
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        p, q = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        loss = loss_fn(p, q)
        w1, w2 = torch.autograd.grad(loss, (p, q))
        for got, want, name in ((res["loss"], loss.detach(), "loss"), (res["g1"], w1, "grad1"), (res["g2"], w2, "grad2")):
            _same_bits(got, want, f"replay {seed} {name}")


# ------------------------------------------------------------------ 7. torch.compile
@pytest.mark.parametrize("border", BORDERS)
def test_compiled_ssim_loss_gives_the_eager_bits(dev, border):
    from networks.ssim_package import SSIMLoss
    shape = (2, 3, TH + 3, TW + 5)
    x, y, m = (t.float().to(dev) for t in R.inputs(shape, "noise", seed=3))
    mask = (m[:, :1] > 0).float()
    loss_fn = SSIMLoss(md=2, border=border)

    def run(fn):
        a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        loss = fn(a, b, mask)
        loss.backward()
        return loss.detach(), a.grad, b.grad

    torch._dynamo.reset()
    want = run(loss_fn)
    got = run(torch.compile(loss_fn, fullgraph=True, backend="aot_eager"))
    for g, w, name in zip(got, want, ("loss", "grad1", "grad2")):
        _same_bits(g, w, f"compiled {name}")


# ------------------------------------------------------------------ last
def test_report_largest_ratios():
    """Not a check: the largest error / bound per quantity and family seen by the tests above, and error / rule bound per quantity."""
    for key in sorted(RATIOS):
        print(f"  {key[0]:6s} {key[1]:10s} largest error / bound {RATIOS[key]:.4f}")
    for key in sorted(RULE):
        print(f"  {key:6s} largest error / rule bound {RULE[key]:.4f}")
