"""The edge-aware smoothness term on the GPU (include/flownet2_hip_smooth.h): the forward and the flow gradient per element against
the float64 reference inside half of the header's bounds, the cells without a term exactly +0, NaN in grad_out where no term is
carried, the L1 form on exactly representable flows, repeated runs and streams bit for bit, strided inputs, autograd, the modules
and ``SmoothnessLoss``.

Every output of a C-ABI call is pre-filled with NaN inside a sentinel-filled allocation that must be untouched afterwards: the
kernels have to write every element of their outputs themselves, and nothing else.

Shapes (N, F, C, H, W): (1, 1, 1, 1, 1), all +0; (1, 2, 3, 2, 2), where order 1 leaves one column and one row and order 2 nothing;
(1, 2, 1, 3, 3), where order 2 leaves exactly one column and one row; (2, 2, 3, 5, 7); (1, 4, 3, 16, 64), exactly one
FN2M_TILE_H x FN2M_TILE_W tile, staged with 16-byte loads; (1, 1, 1, 17, 65), ragged by one both ways; (2, 2, 3, 33, 130), several
tiles both ways, so halos cross tile seams, staged one float at a time; (2, 3, 3, 20, 132), several tiles with 16-byte staging
(W a multiple of 4).  Each with both orders, both edge weightings, eps 0.001 and 0.01 and both image families of smoothness_ref
(alpha 150 on a 5 % image, alpha 10 on a 75 % image: e stays below about 56), on which the fp32 PyTorch composition itself stays
below 0.29 of the bounds.  At the last three shapes also smoothness_ref.inputs' named families -- flushed weights, a ramp whose
second difference cancels, a large offset, graded magnitudes, alpha = 0 -- against the header's bounds in full; the header's
gradient bound is ``backward(..., corrected=True)``'s third array, the original tests keep the first-order bound it replaced.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import fn2_capi
import smoothness_ref as RS

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 64
SHAPES = [(1, 1, 1, 1, 1), (1, 2, 3, 2, 2), (1, 2, 1, 3, 3), (2, 2, 3, 5, 7), (1, 4, 3, 16, 64), (1, 1, 1, 17, 65), (2, 2, 3, 33, 130),
          (2, 3, 3, 20, 132)]
SEAMS, SEAMS_VEC = SHAPES[6], SHAPES[7]
ORDERS = (1, 2)
EPS = (0.001, 0.01)
FAMILIES = (0, 1)
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
    """err <= bound / 2 per element; where the bound is 0 the value is exactly 0.  Prints the largest err / bound first."""
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{what}: largest error / bound {ratio:.4f}")
    assert (got[zero] == 0).all(), f"{what}: not exactly 0 where the bound is 0"
    if ratio > 0.5:
        i = np.unravel_index(np.argmax(np.where(zero, 0, err / np.where(zero, 1, bound))), err.shape)
        raise AssertionError(f"{what}: error {err[i]:.3e} > half of the bound {bound[i]:.3e} at {i} (ratio {ratio:.3f})")


@lru_cache(maxsize=None)
def _inputs(shape, family):
    flow, image, go, alpha = RS.inputs(shape, family, 1000 * shape[3] + 10 * shape[4] + shape[1] + 7 * family)
    for a in (flow, image, go):
        a.setflags(write=False)
    return flow, image, go, alpha


@lru_cache(maxsize=None)
def _case(shape, family, order, edge, eps):
    """Inputs and every reference of one combination, computed once and shared; the arrays are read-only."""
    flow, image, go, alpha = _inputs(shape, family)
    out, fb = RS.forward(flow, image, order, edge, alpha, eps)
    grad, gb = RS.backward(flow, image, go, order, edge, alpha, eps)
    case = dict(flow=flow, image=image, go=go, out=out, fb=fb, grad=grad, gb=gb)
    for v in case.values():
        v.setflags(write=False)
    case["alpha"] = alpha
    return case


def _combos():
    return [(fam, k, edge, eps) for fam in FAMILIES for k in ORDERS for edge in RS.EDGES for eps in EPS]


def _dev(c, dev, *names):
    return [torch.tensor(c[k], device=dev) for k in names]


def _forward(f, im, order, edge, alpha, eps):
    out, whole = _guarded((f.shape[0], 2) + tuple(f.shape[2:]), f.device)
    fn2_capi.smoothness_forward(f, im, order, edge, alpha, eps, out=out)
    torch.cuda.synchronize()
    return out, whole


def _backward(f, im, g, order, edge, alpha, eps):
    grad, whole = _guarded(f.shape, f.device)
    fn2_capi.smoothness_backward(f, im, g, order, edge, alpha, eps, out=grad)
    torch.cuda.synchronize()
    return grad, whole


def _no_term(shape, order, dev):
    """N x 2 x H x W bool: the cells that carry no term (the last k columns of plane 0, the last k rows of plane 1)."""
    N, F, C, H, W = shape
    m = torch.zeros(N, 2, H, W, dtype=torch.bool, device=dev)
    m[:, 0, :, max(W - order, 0):] = True
    m[:, 1, max(H - order, 0):] = True
    return m


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_ids = dict(ids=lambda s: "x".join(map(str, s)))


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_forward_within_half_the_bound(dev, shape):
    """|out - ref| <= half the header's forward bound per element; exactly +0 where the stencil does not fit."""
    N, F, C, H, W = shape
    for fam, order, edge, eps in _combos():
        c = _case(shape, fam, order, edge, eps)
        f, im = _dev(c, dev, "flow", "image")
        out, whole = _forward(f, im, order, edge, c["alpha"], eps)
        what = f"forward {shape} family {fam} order {order} {edge} eps {eps}"
        _untouched(whole, out, what)
        _within(out, c["out"], c["fb"], "forward", what)
        none = _no_term(shape, order, dev)
        assert bool((_bits(out)[none] == 0).all()), f"{what}: a cell without a term is not +0"
        if W > order and H > order:
            assert float(out[~none].min()) > 0
    if shape == (1, 1, 1, 1, 1):
        assert bool(_no_term(shape, 1, dev).all())
    if shape == (1, 2, 3, 2, 2):
        assert int((~_no_term(shape, 1, dev)).sum()) == 4 and bool(_no_term(shape, 2, dev).all())
    if shape == (1, 2, 1, 3, 3):
        assert int((~_no_term(shape, 2, dev)).sum()) == 6


def test_constant_image_and_constant_flow(dev):
    """A constant image gives w = 1 exactly: the output is the sum of rho alone; a constant flow gives w F eps and a zero gradient."""
    shape = SEAMS
    c = _case(shape, 0, 2, "exponential", 0.001)
    f, im, g = _dev(c, dev, "flow", "image", "go")
    flat = torch.full_like(im, 0.375)
    for order in ORDERS:
        for edge in RS.EDGES:
            out, whole = _forward(f, flat, order, edge, 150.0, 0.001)
            _untouched(whole, out, "constant image")
            ref, fb = RS.forward(c["flow"], flat.cpu().numpy(), order, edge, 150.0, 0.001)
            _within(out, ref, fb, "forward", f"constant image order {order} {edge}")
            other, _ = _forward(f, torch.full_like(im, 0.625), order, edge, 7.0, 0.001)
            _same_bits(other, out, "w is not exactly 1 on a constant image")
            const = torch.full_like(f, 3.25)
            grad, gw = _backward(const, im, g, order, edge, 150.0, 0.001)
            _untouched(gw, grad, "constant flow")
            assert bool((grad == 0).all()), "a constant flow has a gradient"
            out, _ = _forward(const, im, order, edge, 150.0, 0.001)
            ref, fb = RS.forward(const.cpu().numpy(), c["image"], order, edge, 150.0, 0.001)
            _within(out, ref, fb, "forward", f"constant flow order {order} {edge}")


# ------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_backward_within_half_the_bound(dev, shape):
    """The flow gradient within half the header's bound and exactly 0 where the bound is 0; NaN in grad_out where no term is
    carried leaves the gradient's bits unchanged; two runs give the same bits."""
    for fam, order, edge, eps in _combos():
        c = _case(shape, fam, order, edge, eps)
        f, im, g = _dev(c, dev, "flow", "image", "go")
        what = f"grad_flow {shape} family {fam} order {order} {edge} eps {eps}"
        grad, whole = _backward(f, im, g, order, edge, c["alpha"], eps)
        _untouched(whole, grad, what)
        _within(grad, c["grad"], c["gb"], "grad_flow", what)
        gn = g.clone()
        gn[_no_term(shape, order, dev)] = float("nan")
        again, whole = _backward(f, im, gn, order, edge, c["alpha"], eps)
        _untouched(whole, again, what + " with NaN in grad_out")
        _same_bits(again, grad, what + ": grad_out is read where no term is carried")
        if eps == EPS[0]:
            again, _ = _backward(f, im, g, order, edge, c["alpha"], eps)
            _same_bits(again, grad, what + ": two runs differ")


def test_l1_form_on_exactly_representable_flows(dev):
    """eps = 0 on flows of multiples of 1/8, |f| <= 64, constant on 5 x 5 patches: every difference is exact, rho' = sign(d) and
    many d are 0.  The forward within half its bound, the gradient within half its bound and exactly 0 where every d reaching the
    pixel is 0."""
    for shape in (SHAPES[3], SEAMS, SEAMS_VEC):
        flow = RS.dyadic_flow(shape, 31, patch=5)
        assert np.abs(flow).max() <= 64 and (flow * 8 == np.rint(flow * 8)).all()
        _, image, go, alpha = _inputs(shape, 0)
        f, im, g = (torch.tensor(a, device=dev) for a in (flow, image, go))
        for order in ORDERS:
            for edge in RS.EDGES:
                what = f"L1 {shape} order {order} {edge}"
                ref, fb = RS.forward(flow, image, order, edge, alpha, 0.0)
                out, whole = _forward(f, im, order, edge, alpha, 0.0)
                _untouched(whole, out, what)
                _within(out, ref, fb, "forward", what)
                gref, gb = RS.backward(flow, image, go, order, edge, alpha, 0.0)
                grad, whole = _backward(f, im, g, order, edge, alpha, 0.0)
                _untouched(whole, grad, what)
                _within(grad, gref, gb, "grad_flow", what)
                # where every reaching d is 0 the reference gradient is a sum of zeros: the kernel's must be 0 too
                reach, _ = RS.backward(flow, image, np.ones_like(go), order, "exponential", 0.0, 0.0)      # w = 1, gO = 1: sum coef sign(d)
                quiet = np.ones(flow.shape, bool)
                for plane, axis in ((0, 3), (1, 2)):
                    q = RS._direction(flow, image, axis, order, edge, alpha, 0.0)
                    if q is None:
                        continue
                    L = flow.shape[axis]
                    for j in range(order + 1):
                        quiet[RS._sl(axis, j, L - order + j)] &= q["d"] == 0
                assert quiet.any() and not quiet.all() and (reach[quiet] == 0).all()
                assert bool((grad.cpu().numpy()[quiet] == 0).all()), f"{what}: a gradient where every reaching d is 0"


# ------------------------------------------------------------------ 3. reproducibility, streams, strides
def test_runs_and_streams_are_bit_identical(dev):
    for shape in (SEAMS, SEAMS_VEC):
        c = _case(shape, 0, 2, "gaussian", 0.001)
        f, im, g = _dev(c, dev, "flow", "image", "go")
        args = (2, "gaussian", c["alpha"], 0.001)
        out, _ = _forward(f, im, *args)
        again, _ = _forward(f, im, *args)
        _same_bits(again, out, "forward: two runs differ")
        grad, _ = _backward(f, im, g, *args)
        again, _ = _backward(f, im, g, *args)
        _same_bits(again, grad, "backward: two runs differ")
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            so, sw = _guarded(out.shape, dev)
            fn2_capi.smoothness_forward(f, im, *args, out=so)
            sg, gw = _guarded(f.shape, dev)
            fn2_capi.smoothness_backward(f, im, g, *args, out=sg)
        side.synchronize()
        for view, whole, want, what in ((so, sw, out, "forward"), (sg, gw, grad, "grad_flow")):
            _untouched(whole, view, what + " on a side stream")
            _same_bits(view, want, what + ": the side stream's result differs")


def test_strided_and_misaligned_inputs_give_the_contiguous_result(dev):
    import smoothness_cuda
    shape = SEAMS_VEC
    c = _case(shape, 0, 2, "exponential", 0.001)
    f, im, g = _dev(c, dev, "flow", "image", "go")
    N, F, C, H, W = shape
    widef, widei = torch.randn(N, F + 2, H, W, device=dev), torch.randn(N, C + 2, H, W, device=dev)
    widef[:, 1:F + 1], widei[:, 1:C + 1] = f, im
    sf, si = widef[:, 1:F + 1], widei[:, 1:C + 1]
    assert not sf.is_contiguous() and not si.is_contiguous()
    want = smoothness_cuda.forward_alloc(f, im, 2)
    _same_bits(smoothness_cuda.forward_alloc(sf, si, 2), want, "forward of channel slices")
    gs = g.transpose(2, 3).contiguous().transpose(2, 3)
    assert not gs.is_contiguous()
    gwant = smoothness_cuda.backward_alloc(f, im, g, 2)
    _same_bits(smoothness_cuda.backward_alloc(sf, si, gs, 2), gwant, "grad_flow of channel slices")
    # a single-channel slice of an RGB image is a grey image
    r = im[:, 0:1]
    assert not r.is_contiguous()
    _same_bits(smoothness_cuda.forward_alloc(f, r, 1), smoothness_cuda.forward_alloc(f, r.contiguous(), 1), "C = 1 slice")
    # tensors that start 4 bytes past a 16-byte boundary take the one-float staging: the same bits as the 16-byte staging
    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=dev)
        buf[1:] = t.flatten()
        v = buf[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    _same_bits(fn2_capi.smoothness_forward(shifted(f), shifted(im), 2), want, "forward of misaligned tensors")
    _same_bits(fn2_capi.smoothness_backward(shifted(f), im, shifted(g), 2), gwant, "grad_flow of misaligned tensors")
    with pytest.raises(RuntimeError, match="gradOutput has shape"):
        smoothness_cuda.backward_alloc(f, im, g[:, :1], 2)


# ------------------------------------------------------------------ 4. autograd and modules
def test_autograd_matches_the_float64_composition(dev):
    """``smoothness_map`` / ``EdgeAwareSmoothness`` through autograd against autograd of the PyTorch composition in float64 -- not
    against this file's numpy reference -- inside half of the bounds."""
    from networks.smoothness_package import EdgeAwareSmoothness, SmoothnessFunction, smoothness_map
    shape = SEAMS
    for order, edge, eps, fam in ((1, "exponential", 0.001, 0), (2, "gaussian", 0.01, 1)):
        c = _case(shape, fam, order, edge, eps)
        f, im, g = _dev(c, dev, "flow", "image", "go")
        alpha = c["alpha"]
        t = torch.from_numpy(c["flow"].astype(np.float64)).requires_grad_(True)
        ref = RS.compose(t, torch.from_numpy(c["image"].astype(np.float64)), order, edge, alpha, eps)
        ref.backward(torch.from_numpy(c["go"].astype(np.float64)))
        x = f.clone().requires_grad_(True)
        out = smoothness_map(x, im, order, edge, alpha, eps)
        assert out.requires_grad and out.shape == (shape[0], 2) + shape[3:]
        _within(out, ref.detach().numpy(), c["fb"], "forward", "smoothness_map against the composition")
        out.backward(g)
        _within(x.grad, t.grad.numpy(), c["gb"], "grad_flow", "autograd grad_flow against the composition")
        raw = fn2_capi.smoothness_backward(f, im, g, order, edge, alpha, eps)
        _same_bits(x.grad, raw, "autograd grad_flow is not the raw call's")
        # the module
        x = f.clone().requires_grad_(True)
        mod = EdgeAwareSmoothness(order, edge, alpha, eps)
        o = mod(x, im)
        _same_bits(o.detach(), out.detach(), "EdgeAwareSmoothness forward")
        o.backward(g)
        _same_bits(x.grad, raw, "EdgeAwareSmoothness gradient")
        assert not smoothness_map(f, im, order, edge, alpha, eps).requires_grad
        # the Function's own static methods give the same node
        x = f.clone().requires_grad_(True)
        super(SmoothnessFunction, SmoothnessFunction).apply(x, im, order, edge, alpha, eps).backward(g)
        _same_bits(x.grad, raw, "SmoothnessFunction.forward / backward")
        # the image gets no gradient, and says so
        with pytest.raises(RuntimeError, match="image requires a gradient"):
            smoothness_map(f, im.clone().requires_grad_(True), order, edge, alpha, eps)


def test_smoothness_loss_matches_its_composition(dev):
    """``SmoothnessLoss`` against UFlow's two means of the float64 composition: the difference is at most the same reduction of
    the per-element bounds plus 64 u of the value for the fp32 sums; its gradient within half the gradient bound."""
    from networks.smoothness_package import SmoothnessLoss
    for shape, order, edge, eps, fam in ((SEAMS, 1, "exponential", 0.001, 0), (SEAMS_VEC, 2, "gaussian", 0.01, 1), (SHAPES[1], 2, "exponential", 0.001, 0)):
        c = _case(shape, fam, order, edge, eps)
        f, im = _dev(c, dev, "flow", "image")
        alpha, F = c["alpha"], shape[1]
        want = float(RS.compose_loss(torch.from_numpy(c["flow"].astype(np.float64)), torch.from_numpy(c["image"].astype(np.float64)), order, edge,
                                     alpha, eps))
        x = f.clone().requires_grad_(True)
        got = SmoothnessLoss(order, edge, alpha, eps)(x, im)
        assert got.dim() == 0
        tol = float(RS.loss_of(c["fb"], F, order)) + 64 * RS.U * abs(want)
        print(f"SmoothnessLoss {shape} order {order}: {float(got.detach())!r} against {want!r}, tolerance {tol:.3e}")
        assert abs(float(got.detach()) - want) <= tol
        got.backward()
        N, _, _, H, W = shape
        go = np.zeros((N, 2, H, W), np.float32)
        if W > order:
            go[:, 0] = np.float32(0.5 / (N * F * H * (W - order)))
        if H > order:
            go[:, 1] = np.float32(0.5 / (N * F * (H - order) * W))
        # (the reduction's own grad_out equals these constants to 1 ulp: 2 u of the bound's 24 u)
        gref, gb = RS.backward(c["flow"], c["image"], go, order, edge, alpha, eps)
        _within(x.grad, gref, gb, "grad_flow", f"SmoothnessLoss gradient {shape}")


# ------------------------------------------------------------------ 5. the named input families, against the bounds in full
FAMILY_SHAPES = [SHAPES[5], SEAMS, SEAMS_VEC]
FAMILY_RATIOS = {}   # (family, quantity) -> largest error / bound seen


def _family_eps(family):
    return RS.GRADED_EPS if family == "graded" else (0.0, 0.001)


@lru_cache(maxsize=None)
def _family_inputs(shape, family):
    flow, image, go, alpha = RS.inputs(shape, family, 1000 * shape[3] + 10 * shape[4] + shape[1] + 7 * RS.NEW_FAMILIES.index(family))
    for a in (flow, image, go):
        a.setflags(write=False)
    return flow, image, go, alpha


def _inside(got, ref, bound, key, what):
    """err <= bound per element, the header's bound with factor 1; where the bound is 0 the value is exactly 0."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(bound).all(), f"{what}: the bound is not finite"
    err = np.abs(got - ref)
    zero = bound == 0
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    FAMILY_RATIOS[key] = max(FAMILY_RATIOS.get(key, 0.0), ratio)
    print(f"{what}: largest error / bound {ratio:.4f}")
    assert (got[zero] == 0).all(), f"{what}: not exactly 0 where the bound is 0"
    if not ratio <= 1.0:
        i = np.unravel_index(np.argmax(np.where(zero, 0, err / np.where(zero, 1, bound))), err.shape)
        raise AssertionError(f"{what}: error {err[i]:.3e} > the bound {bound[i]:.3e} at {i} (ratio {ratio:.3f}): got {got[i]!r}, want {ref[i]!r}")


def _dead_cells(shape, flow, image, order, edge, alpha):
    """N x 2 x H x W bool: the cells whose edge measure is above 104, where exp2's argument is below -150."""
    N, F, C, H, W = shape
    dead = np.zeros((N, 2, H, W), bool)
    for plane, axis in ((0, 3), (1, 2)):
        q = RS._direction(flow, image, axis, order, edge, alpha, 0.0)
        L = (H, W)[axis - 2]
        dead[(slice(None), slice(plane, plane + 1)) + RS._sl(axis, 0, L - order)[2:]] = q["e"] > 104
    return dead


@pytest.mark.parametrize("family", RS.NEW_FAMILIES)
@pytest.mark.parametrize("shape", FAMILY_SHAPES, **_ids)
def test_input_families_within_the_bounds(dev, shape, family):
    """Every named family of smoothness_ref (each asserts its own condition when it is drawn) with both orders and both
    weightings: the forward inside the header's forward bound, the gradient inside the header's gradient bound, both with factor
    1; cells without a term +0; two backward runs the same bits.  ``edges``: a cell with e > 104 is exactly +0 and gives the
    gradient nothing, whatever its grad_out.  ``alpha0`` with eps = 0 on exactly representable flows: the float64 value, exactly."""
    flow, image, go, alpha = _family_inputs(shape, family)
    f, im, g = (torch.tensor(a, device=dev) for a in (flow, image, go))
    for order in ORDERS:
        for edge in RS.EDGES:
            for eps in _family_eps(family):
                what = f"{family} {shape} order {order} {edge} eps {eps:.3g}"
                ref, fb = RS.forward(flow, image, order, edge, alpha, eps)
                gref, _, gb = RS.backward(flow, image, go, order, edge, alpha, eps, corrected=True)
                out, whole = _forward(f, im, order, edge, alpha, eps)
                _untouched(whole, out, what)
                _inside(out, ref, fb, (family, "forward"), "forward " + what)
                assert bool((_bits(out)[_no_term(shape, order, dev)] == 0).all()), f"{what}: a cell without a term is not +0"
                grad, whole = _backward(f, im, g, order, edge, alpha, eps)
                _untouched(whole, grad, what)
                _inside(grad, gref, gb, (family, "grad_flow"), "grad_flow " + what)
                if eps == _family_eps(family)[-1]:
                    again, _ = _backward(f, im, g, order, edge, alpha, eps)
                    _same_bits(again, grad, what + ": two runs differ")
                if family == "edges":
                    dead = _dead_cells(shape, flow, image, order, edge, alpha)
                    assert dead.any() and not dead.all()
                    dead_d = torch.tensor(dead, device=dev)
                    assert bool((_bits(out)[dead_d] == 0).all()), f"{what}: a cell with e > 104 is not +0"
                    tripled, _ = _backward(f, im, torch.where(dead_d, 3 * g, g), order, edge, alpha, eps)
                    _same_bits(tripled, grad, what + ": grad_out of a cell with e > 104 reaches the gradient")
                    without, _ = _backward(f, im, torch.where(dead_d, torch.zeros_like(g), g), order, edge, alpha, eps)
                    assert bool((without == grad).all()), f"{what}: a cell with e > 104 contributes to the gradient"
                if family == "alpha0" and eps == 0.0:
                    emu, _ = RS.emulate(flow, image, go, order, edge, alpha, eps)
                    assert np.array_equal(emu.astype(np.float64), ref)      # every rho and their sum are exact
                    _same_bits(out, torch.tensor(emu, device=dev), what + ": not sum_f rho exactly with alpha = 0")


def test_report_largest_ratios():
    """Last: the largest error / bound ratios of this run, for DESIGN 4.15."""
    for key in sorted(RATIOS):
        print("largest error / bound", key, f"{RATIOS[key]:.4f}")
    for family, quantity in sorted(FAMILY_RATIOS):
        print("largest error / bound, family", family, quantity, f"{FAMILY_RATIOS[family, quantity]:.4f}")
    assert set(RATIOS) == {"forward", "grad_flow"} and max(RATIOS.values()) <= 0.5
    assert set(FAMILY_RATIOS) == {(fam, q) for fam in RS.NEW_FAMILIES for q in ("forward", "grad_flow")} and max(FAMILY_RATIOS.values()) <= 1.0
