"""The ternary census distance on the GPU (include/flownet2_hip_census.h): the forward and both gradients per element against the
float64 reference inside a quarter of the header's bounds, the border ring and the small images exactly, the gradient asked for
alone and the repeated run bit for bit, autograd, the modules and ``CensusLoss``.

Every output of a C-ABI call is pre-filled with NaN inside a sentinel-filled allocation that must be untouched afterwards: the
kernels have to write every element of their outputs themselves, and nothing else.

Shapes (N, C, H, W): (1, 1, 1, 1); (1, 1, 7, 7), where max_distance 3 leaves exactly one interior pixel; (2, 3, 5, 7), where
max_distance 3 leaves nothing; (1, 1, 17, 67), ragged against the FN2C_TILE_H x FN2C_TILE_W = 16 x 64 tile both ways;
(2, 3, 33, 130), several tiles both ways, so halos cross tile seams.  Each with max_distance 1, 2, 3 and normalize on and off.
Inputs: census_ref.image_pair -- im1 uniform, im2 = im1 + 5 % noise -- on which the fp32 PyTorch composition itself stays below
0.03 of the bounds, so a quarter of the bound is far from the reference's own error.  At the two larger shapes also
census_ref.image_family's families at their scales -- low contrast, opposed images, a flat pair, graded magnitudes, transitions on
the tile seams, negative, unit and tiny scales -- against the bounds in full.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import census_ref as RC
import fn2_capi

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 64
SHAPES = [(1, 1, 1, 1), (1, 1, 7, 7), (2, 3, 5, 7), (1, 1, 17, 67), (2, 3, 33, 130)]
MDS = [1, 2, 3]
SCALE = 255.0
RATIOS = {}   # quantity -> largest error / bound seen, printed by the last test


# ------------------------------------------------------------------ helpers
def _guarded(shape, dev):
    n = int(np.prod(shape))
    whole = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = whole[GUARD:GUARD + n].view(shape)
    view.fill_(float("nan"))
    return view, whole


def _untouched(whole, view, what):
    n, lo = view.numel(), view.storage_offset()
    assert bool((whole[:lo] == SENTINEL).all()) and bool((whole[lo + n:] == SENTINEL).all()), f"{what}: wrote outside its output"
    assert not bool(torch.isnan(view).any()), f"{what}: left or produced NaN"


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


def _within(got, ref, bound, key, what):
    """err <= bound / 4 per element; where the bound is 0 the value is exactly 0.  Prints the largest err / bound first."""
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{what}: largest error / bound {ratio:.4f}")
    assert (got[zero] == 0).all(), f"{what}: not exactly 0 where the bound is 0"
    if ratio > 0.25:
        i = np.unravel_index(np.argmax(np.where(zero, 0, err / np.where(zero, 1, bound))), err.shape)
        raise AssertionError(f"{what}: error {err[i]:.3e} > a quarter of the bound {bound[i]:.3e} at {i} (ratio {ratio:.3f})")


@lru_cache(maxsize=None)
def _inputs(shape):
    c = RC.image_pair(shape, 1000 * shape[2] + 10 * shape[3] + shape[1])
    for a in c:
        a.setflags(write=False)
    return c


@lru_cache(maxsize=None)
def _case(shape, md, normalize):
    """Inputs and every reference of one (shape, md, normalize), computed once and shared; the arrays are read-only."""
    im1, im2, go = _inputs(shape)
    out = RC.forward(im1, im2, md, SCALE, normalize)
    g1, g2, A = RC.backward(im1, im2, go, md, SCALE, normalize)
    case = dict(im1=im1, im2=im2, go=go, out=out, g1=g1, g2=g2, A=A)
    for v in case.values():
        v.setflags(write=False)
    return case


def _dev(c, dev, *names):
    return [torch.tensor(c[k], device=dev) for k in names]


def _forward(a, b, md, normalize):
    out, whole = _guarded((a.shape[0], 1) + tuple(a.shape[2:]), a.device)
    fn2_capi.census_forward(a, b, md, SCALE, normalize, out=out)
    torch.cuda.synchronize()
    return out, whole


def _backward(a, b, g, md, normalize, want1=True, want2=True):
    g1, w1 = _guarded(a.shape, a.device)
    g2, w2 = _guarded(a.shape, a.device)
    r1, r2 = fn2_capi.census_backward(a, b, g, md, SCALE, normalize, want1, want2, grads=(g1, g2))
    torch.cuda.synchronize()
    return (r1, w1, g1), (r2, w2, g2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_ids = dict(ids=lambda s: "x".join(map(str, s)))


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_forward_within_a_quarter_of_the_bound(dev, shape):
    """|out - ref| <= 2^-19 w K / 4 per pixel; exactly +0 on the border ring, and everywhere in an image smaller than the patch."""
    N, C, H, W = shape
    for md in MDS:
        ring = torch.from_numpy(~RC.inner(H, W, md)).to(dev)
        for normalize in (True, False):
            c = _case(shape, md, normalize)
            a, b = _dev(c, dev, "im1", "im2")
            out, whole = _forward(a, b, md, normalize)
            what = f"forward {shape} md {md} normalize {normalize}"
            _untouched(whole, out, what)
            _within(out, c["out"], RC.forward_bound(md, normalize), "forward", what)
            assert bool((_bits(out)[:, 0][:, ring] == 0).all()), f"{what}: the border ring is not +0"
            if H < 2 * md + 1 or W < 2 * md + 1:
                assert bool((_bits(out) == 0).all()), f"{what}: an image smaller than the patch is not all +0"
            else:
                assert float(out[:, 0][:, ~ring].min()) > 0
    if shape == (1, 1, 7, 7):
        assert int(RC.inner(7, 7, 3).sum()) == 1


def test_identical_and_brightened_images_give_zero(dev):
    shape = SHAPES[4]
    im1, _, go = _inputs(shape)
    a, g = torch.tensor(im1, device=dev), torch.tensor(go, device=dev)
    # the same brightness step on integer grey levels: every difference is the same float in both images
    grey = torch.from_numpy(np.rint(RC.grey(im1, SCALE)))[:, None].to(dev)
    for md in MDS:
        out, whole = _forward(a, a.clone(), md, True)
        _untouched(whole, out, "identical images")
        assert bool((_bits(out) == 0).all())
        (g1, w1, _), (g2, w2, _) = _backward(a, a.clone(), g, md, True)
        _untouched(w1, g1, "identical images grad1")
        _untouched(w2, g2, "identical images grad2")
        assert bool((g1 == 0).all()) and bool((g2 == 0).all())
        out = fn2_capi.census_forward(grey, grey + 17.0, md, 1.0, False)
        assert bool((out == 0).all()), "census is not brightness-invariant"


# ------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_backward_within_a_quarter_of_the_bounds(dev, shape):
    """Both gradients within 2^-15 A(q, c) / 4 and exactly 0 where A = 0; each gradient asked for alone has the pair's bits; two
    runs give the same bits."""
    for md in MDS:
        for normalize in (True, False):
            c = _case(shape, md, normalize)
            a, b, g = _dev(c, dev, "im1", "im2", "go")
            what = f"{shape} md {md} normalize {normalize}"
            (g1, w1, _), (g2, w2, _) = _backward(a, b, g, md, normalize)
            _untouched(w1, g1, "grad_im1 " + what)
            _untouched(w2, g2, "grad_im2 " + what)
            bound = RC.backward_bound(c["A"])
            _within(g1, c["g1"], bound, "grad_im1", "grad_im1 " + what)
            _within(g2, c["g2"], bound, "grad_im2", "grad_im2 " + what)
            (o1, w1, _), (none, w2, buf2) = _backward(a, b, g, md, normalize, want2=False)
            assert none is None and bool(torch.isnan(buf2).all()), "the gradient that was not wanted was written"
            _untouched(w1, o1, "grad_im1 alone " + what)
            _same_bits(o1, g1, "grad_im1 alone differs from the pair " + what)
            (none, w1, buf1), (o2, w2, _) = _backward(a, b, g, md, normalize, want1=False)
            assert none is None and bool(torch.isnan(buf1).all()), "the gradient that was not wanted was written"
            _untouched(w2, o2, "grad_im2 alone " + what)
            _same_bits(o2, g2, "grad_im2 alone differs from the pair " + what)
            (r1, _, _), (r2, _, _) = _backward(a, b, g, md, normalize)
            _same_bits(r1, g1, "grad_im1: two runs differ " + what)
            _same_bits(r2, g2, "grad_im2: two runs differ " + what)


def test_grad_out_on_the_ring_reaches_no_gradient(dev):
    shape = SHAPES[4]
    N, C, H, W = shape
    for md in MDS:
        c = _case(shape, md, True)
        a, b, g = _dev(c, dev, "im1", "im2", "go")
        ring = torch.from_numpy(~RC.inner(H, W, md)).to(dev)
        (g1, _, _), (g2, _, _) = _backward(a, b, (g * ring).contiguous(), md, True)
        assert float((g * ring).abs().max()) > 0 and bool((g1 == 0).all()) and bool((g2 == 0).all())
        (f1, _, _), (f2, _, _) = _backward(a, b, g, md, True)
        (i1, _, _), (i2, _, _) = _backward(a, b, (g * ~ring).contiguous(), md, True)
        _same_bits(i1, f1, "grad_im1 depends on grad_out on the ring")
        _same_bits(i2, f2, "grad_im2 depends on grad_out on the ring")


# ------------------------------------------------------------------ 3. reproducibility, streams, strides
def test_runs_and_streams_are_bit_identical(dev):
    shape = SHAPES[4]
    c = _case(shape, 3, True)
    a, b, g = _dev(c, dev, "im1", "im2", "go")
    out, _ = _forward(a, b, 3, True)
    again, _ = _forward(a, b, 3, True)
    _same_bits(again, out, "forward: two runs differ")
    (g1, _, _), (g2, _, _) = _backward(a, b, g, 3, True)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        so, sw = _guarded(out.shape, dev)
        fn2_capi.census_forward(a, b, 3, SCALE, True, out=so)
        s1, w1 = _guarded(a.shape, dev)
        s2, w2 = _guarded(a.shape, dev)
        fn2_capi.census_backward(a, b, g, 3, SCALE, True, grads=(s1, s2))
    side.synchronize()
    for view, whole, want, what in ((so, sw, out, "forward"), (s1, w1, g1, "grad_im1"), (s2, w2, g2, "grad_im2")):
        _untouched(whole, view, what + " on a side stream")
        _same_bits(view, want, what + ": the side stream's result differs")


def test_channel_sliced_input_gives_the_contiguous_result(dev):
    import census_cuda
    shape = SHAPES[4]
    c = _case(shape, 2, True)
    a, b, g = _dev(c, dev, "im1", "im2", "go")
    wide1, wide2 = torch.randn(shape[0], 5, *shape[2:], device=dev), torch.randn(shape[0], 5, *shape[2:], device=dev)
    wide1[:, 1:4], wide2[:, 1:4] = a, b
    s1, s2 = wide1[:, 1:4], wide2[:, 1:4]
    assert not s1.is_contiguous() and not s2.is_contiguous()
    _same_bits(census_cuda.forward_alloc(s1, s2, 2), census_cuda.forward_alloc(a, b, 2), "forward of channel slices")
    gs = g.expand(-1, 1, -1, -1).transpose(2, 3).contiguous().transpose(2, 3)
    assert not gs.is_contiguous()
    got, want = census_cuda.backward_alloc(s1, s2, gs, 2), census_cuda.backward_alloc(a, b, g, 2)
    _same_bits(got[0], want[0], "grad_im1 of channel slices")
    _same_bits(got[1], want[1], "grad_im2 of channel slices")
    # a single-channel slice of an RGB image is a grey image
    r1, r2 = a[:, 0:1], b[:, 0:1]
    assert not r1.is_contiguous()
    _same_bits(census_cuda.forward_alloc(r1, r2, 2), census_cuda.forward_alloc(r1.contiguous(), r2.contiguous(), 2), "C = 1 slice")


# ------------------------------------------------------------------ 4. autograd and modules
def test_autograd_matches_the_float64_composition(dev):
    """``census_distance`` / ``TernaryCensus`` through autograd against autograd of the composition in float64 on the fp32 grey
    intensities -- not against this file's reference -- inside a quarter of the bounds."""
    from networks.census_package import CensusFunction, TernaryCensus, census_distance
    shape, md = SHAPES[4], 3
    c = _case(shape, md, True)
    a, b, g = _dev(c, dev, "im1", "im2", "go")
    t1, t2 = (torch.from_numpy(RC.grey(c[k], SCALE).astype(np.float64))[:, None].requires_grad_(True) for k in ("im1", "im2"))
    ref = RC.compose_grey(t1, t2, md, True)
    ref.backward(torch.from_numpy(c["go"].astype(np.float64)))
    cw = torch.tensor([float(v) for v in RC.CW], dtype=torch.float64).view(1, 3, 1, 1) * float(np.float32(SCALE))
    ref1, ref2 = (cw * t1.grad).numpy(), (cw * t2.grad).numpy()
    bound = RC.backward_bound(c["A"])
    x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = census_distance(x, y, md)
    _within(out, ref.detach().numpy(), RC.forward_bound(md), "forward", "census_distance against the composition")
    out.backward(g)
    _within(x.grad, ref1, bound, "grad_im1", "autograd grad_im1 against the composition")
    _within(y.grad, ref2, bound, "grad_im2", "autograd grad_im2 against the composition")
    g1, g2 = fn2_capi.census_backward(a, b, g, md, SCALE, True)
    _same_bits(x.grad, g1, "autograd grad_im1 is not the raw call's")
    _same_bits(y.grad, g2, "autograd grad_im2 is not the raw call's")
    # the module, and needs_input_grad: one gradient only
    x = a.clone().requires_grad_(True)
    mod = TernaryCensus(md)
    o = mod(x, b)
    _same_bits(o.detach(), out.detach(), "TernaryCensus forward")
    o.backward(g)
    _same_bits(x.grad, g1, "im1-only gradient")
    y = b.clone().requires_grad_(True)
    CensusFunction.apply(a, y, md).backward(g)
    _same_bits(y.grad, g2, "im2-only gradient")
    assert not census_distance(a, b, md).requires_grad
    # the sum instead of the mean, another scale
    s = census_distance(a, b, 2, 100.0, False)
    _within(s, RC.forward(c["im1"], c["im2"], 2, 100.0, False), RC.forward_bound(2, False), "forward", "census_distance sum, scale 100")
    # the Function's own static methods give the same node
    x = a.clone().requires_grad_(True)
    super(CensusFunction, CensusFunction).apply(x, b, md, SCALE, True).backward(g)
    _same_bits(x.grad, g1, "CensusFunction.forward / backward")


def test_census_loss_matches_its_composition(dev):
    from networks.census_package import CensusLoss
    shape = SHAPES[4]
    im1, im2, _ = _inputs(shape)
    a, b = torch.tensor(im1, device=dev), torch.tensor(im2, device=dev)
    t1, t2 = (torch.from_numpy(RC.grey(im, SCALE).astype(np.float64))[:, None] for im in (im1, im2))      # float64 from the fp32 grey
    mask = torch.from_numpy((np.random.default_rng(3).random((shape[0], 1) + shape[2:]) > 0.3).astype(np.float32)).to(dev)
    for md in (1, 3):
        loss = CensusLoss(md)
        for m in (None, mask):
            x = a.clone().requires_grad_(True)
            got = loss(x, b, m)
            want = RC.compose_loss(t1, t2, None if m is None else m.cpu().double(), md)
            assert got.dim() == 0 and abs(float(got.detach()) - float(want)) <= 1e-5 * abs(float(want)), (md, float(got.detach()), float(want))
            got.backward()
            assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="must be N x 1 x H x W"):
        CensusLoss(3)(a, b, mask[:, :, 1:])


# ------------------------------------------------------------------ 5. the image families, against the bounds in full
FAMILY_SHAPES = [SHAPES[3], SHAPES[4]]
FAMILY_MDS = (1, 3)
FAMILY_RATIOS = {}   # (family, scale, quantity) -> largest error / bound seen


@lru_cache(maxsize=None)
def _family_inputs(shape, family):
    seed = 1000 * shape[2] + 10 * shape[3] + shape[1] + 7 * RC.FAMILIES.index(family)
    im1, im2, _ = RC.image_family(family, shape, seed)
    go = RC.grad_out(shape, seed + 1)
    for a in (im1, im2, go):
        a.setflags(write=False)
    return im1, im2, go


def _inside(got, ref, bound, key, what):
    """err <= bound per element, the header's bound with factor 1; finite; where the bound is 0 the value is exactly 0."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    FAMILY_RATIOS[key] = max(FAMILY_RATIOS.get(key, 0.0), ratio)
    print(f"{what}: largest error / bound {ratio:.4f}")
    assert (got[zero] == 0).all(), f"{what}: not exactly 0 where the bound is 0"
    if not ratio <= 1.0:
        i = np.unravel_index(np.argmax(np.where(zero, 0, err / np.where(zero, 1, bound))), err.shape)
        raise AssertionError(f"{what}: error {err[i]:.3e} > the bound {bound[i]:.3e} at {i} (ratio {ratio:.3f}): got {got[i]!r}, want {ref[i]!r}")


@pytest.mark.parametrize("family,scale", RC.FAMILY_SCALES, ids=lambda v: v if isinstance(v, str) else f"{v:g}")
@pytest.mark.parametrize("shape", FAMILY_SHAPES, **_ids)
def test_image_families_within_the_bounds(dev, shape, family, scale):
    """Every family of census_ref (each asserts its own condition when it is drawn) at its scales, max_distance 1 and 3, normalize
    on and off: the forward inside 2^-19 w K and both gradients inside 2^-15 A(q, c), factor 1; finite everywhere; exactly +0 on the
    ring and exactly 0 where A = 0; the repeated run bit for bit."""
    N, C, H, W = shape
    im1, im2, go = _family_inputs(shape, family)
    a, b, g = (torch.tensor(v, device=dev) for v in (im1, im2, go))
    for md in FAMILY_MDS:
        ring = torch.from_numpy(~RC.inner(H, W, md)).to(dev)
        for normalize in (True, False):
            what = f"{family} scale {scale:g} {shape} md {md} normalize {normalize}"
            ref = RC.forward(im1, im2, md, scale, normalize)
            r1, r2, A = RC.backward(im1, im2, go, md, scale, normalize)
            assert np.isfinite(ref).all() and np.isfinite(r1).all() and np.isfinite(r2).all() and np.isfinite(A).all()
            outs = []
            for _ in range(2):
                out, whole = _guarded((N, 1, H, W), dev)
                fn2_capi.census_forward(a, b, md, scale, normalize, out=out)
                g1, w1 = _guarded(shape, dev)
                g2, w2 = _guarded(shape, dev)
                fn2_capi.census_backward(a, b, g, md, scale, normalize, True, True, grads=(g1, g2))
                torch.cuda.synchronize()
                for view, buf, name in ((out, whole, "forward"), (g1, w1, "grad_im1"), (g2, w2, "grad_im2")):
                    _untouched(buf, view, f"{name} {what}")
                outs.append((out, g1, g2))
            (out, g1, g2), again = outs
            for x, y, name in zip(outs[0], again, ("forward", "grad_im1", "grad_im2")):
                _same_bits(y, x, f"{name} {what}: two runs differ")
            _inside(out, ref, RC.forward_bound(md, normalize), (family, scale, "forward"), "forward " + what)
            assert bool((_bits(out)[:, 0][:, ring] == 0).all()), f"{what}: the border ring is not +0"
            bound = RC.backward_bound(A)
            assert (bound > 0).any()
            _inside(g1, r1, bound, (family, scale, "grad_im1"), "grad_im1 " + what)
            _inside(g2, r2, bound, (family, scale, "grad_im2"), "grad_im2 " + what)


def test_report_largest_ratios():
    """Last: the largest error / bound ratios of this run, for DESIGN 4.14."""
    for key in sorted(RATIOS):
        print("largest error / bound", key, f"{RATIOS[key]:.4f}")
    for family, scale, quantity in sorted(FAMILY_RATIOS):
        print("largest error / bound, family", family, f"scale {scale:g}", quantity, f"{FAMILY_RATIOS[family, scale, quantity]:.4f}")
    assert set(RATIOS) == {"forward", "grad_im1", "grad_im2"} and max(RATIOS.values()) <= 0.25
    assert set(FAMILY_RATIOS) == {(f, s, q) for f, s in RC.FAMILY_SCALES for q in ("forward", "grad_im1", "grad_im2")}
    assert max(FAMILY_RATIOS.values()) <= 1.0
