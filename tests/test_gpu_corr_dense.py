"""The dense stride-1 correlation kernels (csrc/correlation_dense.hip): Correlation(md, 1, md, 1, 1), 1 <= md <= 4, PWC-Net's
cost volume, on float, half and bfloat16 tensors.

Their contract is the general kernel's bits: every element equals what FN2_CORR_DIRECT produces for the same call, bit pattern
for bit pattern -- forward, fused forward and both gradients, through every door (the debug variant that names the kernels,
FN2_CORR_AUTO at the C ABI, the pybind module, the autograd modules).  Elements that are NaN in the general kernel's result are
compared for NaN-ness only (a payload is no part of the contract); they must be at most 5 % of a tensor.  Independently of the
general kernel the results lie in the float64 brackets of the documented FN2_CORR_DIRECT bounds, which pins the general kernel
on dense parameters too.  Bits cannot tell which kernel ran: the debug variant's return code and a timing comparison do.

FN2_CORR_AUTO takes the tiled FORWARD only from 192 workgroups (batch x tiles of 32 x 4 pixels) up -- on smaller problems the
general kernel is measured faster -- so on most shapes here AUTO's forward is the general kernel and the debug
variant is what reaches the tiled one; (8, 32, 96, 128) and the timing test's shapes are above the gate.  The backward is tiled
at every size."""
import pytest
import torch

import corr_contract_ref as R
import lowp_ref as L

pytestmark = pytest.mark.gpu

SLOPE = 0.1
EUNSUPPORTED = "code -4"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
IDS = ["f32", "half", "bf16"]
NAN_LIMIT = 0.05

# (md, (B, C, H, W)); BIG runs input families 1 and 9 only
BIG = (8, 32, 96, 128)
CASES = [(4, (2, 34, 18, 24)), (4, (1, 196, 6, 8)), (4, (1, 64, 48, 64)), (4, (3, 7, 5, 7)), (4, (1, 1, 1, 1)), (4, (1, 16, 9, 130)),
         (4, BIG), (3, (2, 32, 17, 70)), (2, (2, 20, 33, 31)), (1, (1, 5, 16, 9))]
MISALIGNED = [(2, 10, 11, 13), (2, 10, 11, 14)]   # md 4, run on views that start one element past a 16-byte boundary


def _params(md):
    return (md, 1, md, 1, 1)


def _families(shape, dtype):
    fams = list(R.FAMILIES) if dtype == F32 else [1, 2, 3, 4, 5]
    if shape == BIG:
        fams = [f for f in fams if f in (1, 9)]
    if shape == (1, 1, 1, 1):
        fams = [f for f in fams if f != 9]   # its single pixel would be all NaN
    return fams


def _inputs(fam, shape, dtype, seed):
    return R.family_inputs(fam, shape, seed) if dtype == F32 else L.family_inputs(fam, shape, dtype, seed)


def _kinds(dtype):
    return ("normal", "leaky", "window") + (("planes", "train") if dtype == F32 else ())


def _gout(kind, shape, dtype, seed):
    return R.grad_output(kind, shape, seed) if dtype == F32 else L.grad_output(kind, shape, dtype, seed)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _nan(shape, dtype, dev, off=0):
    """A NaN-filled tensor; off = 1: a view that starts one element into its allocation."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + off,), float("nan"), dtype=dtype, device=dev)
    return flat[off:].view(shape)


def _place(t, dev, off=0):
    if not off:
        return t.to(dev)
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    v = flat[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * t.element_size()
    return v


def _same_bits(got, direct, what):
    """got == direct bit for bit, except that where the general kernel's result is NaN the other must be NaN (any payload)."""
    assert got.shape == direct.shape and got.dtype == direct.dtype, what
    nan = torch.isnan(direct)
    frac = float(nan.double().mean()) if nan.numel() else 0.0
    assert frac <= NAN_LIMIT, f"{what}: {frac:.3%} of the general kernel's elements are NaN"
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN elements differ from the general kernel's"
    gb, db = _bits(got), _bits(direct)
    bad = (gb != db) & ~nan
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ from FN2_CORR_DIRECT; first at flat index {i}: "
                             f"{float(got.flatten()[i])!r} vs {float(direct.flatten()[i])!r}")


def _in_bracket(got, ref, delta, dtype, nonfinite, what, post=None):
    """Finite elements inside the bracket of the float64 reference; non-finite ones exactly where a term is not finite."""
    fin = ~nonfinite
    assert torch.equal(torch.isfinite(got), fin), f"{what}: non-finite outputs differ from the float64 reference's"
    lo, hi = L.bracket(ref[fin], delta[fin], dtype, post=post)
    L.check_bracket(got[fin], lo, hi, what)


def _fwd_delta(ref, absr, C, dtype):
    return {F32: R.delta_direct_f32, F16: L.delta_fwd_direct_half, BF16: L.delta_fwd}[dtype](ref, absr, C)


def _bwd_delta(ref, absr, md, dtype):
    if dtype == F32:
        return R.delta_direct_bwd_f32(ref, absr, L.n_bwd(md, 1, 1))
    return L.delta_bwd(ref, absr, md=md, s2=1, k=1)


def _structural_zeros(H, W, md, dev):
    """(1, D*D, H, W) mask of outputs whose displaced pixel lies in the padding."""
    ys, xs = torch.arange(H, device=dev)[:, None], torch.arange(W, device=dev)[None, :]
    planes = []
    for dy in range(-md, md + 1):
        for dx in range(-md, md + 1):
            planes.append(~((ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W)))
    return torch.stack(planes)[None]


def _forward_case(dev, md, shape, dtype, fam, off=0):
    import correlation_cuda
    import fn2_capi
    from networks.correlation_package.correlation import Correlation, CorrelationLeakyReLUCat
    params = _params(md)
    B, C, H, W = shape
    what = f"fwd md {md} {shape} {dtype} family {fam}"
    a, b = _inputs(fam, shape, dtype, seed=sum(shape) + md)
    ad, bd = _place(a, dev, off), _place(b, dev, off)
    oshape = (B,) + L.out_shape(H, W, *params)
    nOut = oshape[1]
    direct = fn2_capi.correlation_forward(ad, bd, *params, algo=fn2_capi.FN2_CORR_DIRECT, out=_nan(oshape, dtype, dev, off))
    if not (torch.isnan(ad).any() or torch.isnan(bd).any() or torch.isinf(ad).any()):
        assert not torch.isnan(direct).any(), f"{what}: the general kernel left elements unwritten"
    # 1. bits, through every door
    dense = fn2_capi.correlation_forward(ad, bd, *params, algo=fn2_capi.FN2_DEBUG_CORR_DENSE, out=_nan(oshape, dtype, dev, off))
    _same_bits(dense, direct, what + " debug variant")
    auto = fn2_capi.correlation_forward(ad, bd, *params, out=_nan(oshape, dtype, dev, off))
    _same_bits(auto, direct, what + " AUTO (C ABI)")
    e1, e2, o = (torch.empty(0, dtype=dtype, device=dev) for _ in range(3))
    correlation_cuda.forward(ad, bd, e1, e2, o, *params, 1)
    _same_bits(o, direct, what + " correlation_cuda.forward")
    ar, br = ad.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    mod = Correlation(*params)(ar, br)
    _same_bits(mod.detach(), direct, what + " Correlation module")
    # fused: channel offset 8, slope 0.1, three spare channels behind the slice; nothing outside the slice may change
    g = torch.Generator(device=dev).manual_seed(B + C + H + W)
    buf0 = torch.randn((B, 8 + nOut + 3, H, W), generator=g, device=dev).to(dtype)
    buf0[:, 8:8 + nOut] = float("nan")
    fdirect = fn2_capi.correlation_forward_fused(ad, bd, buf0.clone(), 8, SLOPE, *params, algo=fn2_capi.FN2_CORR_DIRECT)
    assert torch.equal(_bits(fdirect[:, :8]), _bits(buf0[:, :8])) and torch.equal(_bits(fdirect[:, 8 + nOut:]), _bits(buf0[:, 8 + nOut:]))
    fauto = fn2_capi.correlation_forward_fused(ad, bd, buf0.clone(), 8, SLOPE, *params)
    fpy = buf0.clone()
    correlation_cuda.forward_fused(ad, bd, fpy, 8, SLOPE, *params)
    for name, fb in (("AUTO (C ABI)", fauto), ("correlation_cuda.forward_fused", fpy)):
        assert torch.equal(_bits(fb[:, :8]), _bits(buf0[:, :8])), f"{what} fused {name}: channels in front of the slice changed"
        assert torch.equal(_bits(fb[:, 8 + nOut:]), _bits(buf0[:, 8 + nOut:])), f"{what} fused {name}: channels behind the slice changed"
        _same_bits(fb[:, 8:8 + nOut], fdirect[:, 8:8 + nOut], f"{what} fused {name}")
    cat = CorrelationLeakyReLUCat(*params, negative_slope=SLOPE)(ad, bd, buf0[:, :8].contiguous())
    assert torch.equal(_bits(cat[:, :8]), _bits(buf0[:, :8]))
    _same_bits(cat[:, 8:], fdirect[:, 8:8 + nOut], what + " CorrelationLeakyReLUCat")
    # 2. independent of the general kernel: the float64 bracket of the documented bound; all-padding outputs exactly zero
    nonfin = R.fwd_nonfinite(ad, bd, params)
    a64, b64 = R.finite_part(ad.double()), R.finite_part(bd.double())
    ref, absr = L.corr_fwd64(a64, b64, *params), L.corr_fwd64(a64.abs(), b64.abs(), *params)
    delta = _fwd_delta(ref, absr, C, dtype)
    _in_bracket(dense, ref, delta, dtype, nonfin, what)
    _in_bracket(fauto[:, 8:8 + nOut], ref, delta, dtype, nonfin, what + " fused", post=L.leaky_general(SLOPE, dtype))
    zeros = _structural_zeros(H, W, md, dev).expand_as(dense)
    assert bool((dense[zeros] == 0).all()) and bool((direct[zeros] == 0).all()), f"{what}: an all-padding output is not exactly zero"
    return ad, bd, fdirect


def _backward_case(dev, md, shape, dtype, fam, ad, bd, fdirect, off=0):
    import correlation_cuda
    import fn2_capi
    from networks.correlation_package.correlation import Correlation, CorrelationLeakyReLUCat
    params = _params(md)
    B, C, H, W = shape
    oshape = (B,) + L.out_shape(H, W, *params)
    nOut = oshape[1]
    a64, b64 = R.finite_part(ad.double()), R.finite_part(bd.double())
    for kind in _kinds(dtype):
        what = f"bwd md {md} {shape} {dtype} family {fam} gradOutput {kind}"
        gd = _place(_gout(kind, oshape, dtype, seed=fam + md), dev, off)
        outs = lambda: (_nan(shape, dtype, dev, off), _nan(shape, dtype, dev, off))   # noqa: E731
        d1, d2 = fn2_capi.correlation_backward(ad, bd, gd, *params, algo=fn2_capi.FN2_CORR_DIRECT, out=outs())
        s1, s2 = fn2_capi.correlation_backward(ad, bd, gd, *params, algo=fn2_capi.FN2_DEBUG_CORR_DENSE, out=outs())
        _same_bits(s1, d1, what + " debug variant grad_input1")
        _same_bits(s2, d2, what + " debug variant grad_input2")
        a1, a2 = fn2_capi.correlation_backward(ad, bd, gd, *params, out=outs())
        _same_bits(a1, d1, what + " AUTO (C ABI) grad_input1")
        _same_bits(a2, d2, what + " AUTO (C ABI) grad_input2")
        e1, e2, p1, p2 = (torch.empty(0, dtype=dtype, device=dev) for _ in range(4))
        correlation_cuda.backward(ad, bd, e1, e2, gd, p1, p2, *params, 1)
        _same_bits(p1, d1, what + " correlation_cuda.backward grad_input1")
        _same_bits(p2, d2, what + " correlation_cuda.backward grad_input2")
        ar, br = ad.clone().requires_grad_(True), bd.clone().requires_grad_(True)
        Correlation(*params)(ar, br).backward(gd)
        _same_bits(ar.grad, d1, what + " Correlation module grad_input1")
        _same_bits(br.grad, d2, what + " Correlation module grad_input2")
        # the float64 brackets
        nf1, nf2 = R.bwd_nonfinite(ad, bd, gd, params)
        r1, r2 = L.corr_bwd64(a64, b64, gd, *params)
        ab1, ab2 = L.corr_bwd64(a64.abs(), b64.abs(), gd.abs(), *params)
        _in_bracket(s1, r1, _bwd_delta(r1, ab1, md, dtype), dtype, nf1, what + " grad_input1")
        _in_bracket(s2, r2, _bwd_delta(r2, ab2, md, dtype), dtype, nf2, what + " grad_input2")
        if kind != "normal":
            continue
        # the fused backward: the mask pass, then the same kernels
        what = f"fused bwd md {md} {shape} {dtype} family {fam}"
        gbuf = torch.zeros_like(fdirect)
        gbuf[:, 8:8 + nOut] = gd
        f1, f2 = fn2_capi.correlation_backward_fused(ad, bd, fdirect, gbuf, 8, SLOPE, *params, algo=fn2_capi.FN2_CORR_DIRECT)
        x1, x2 = fn2_capi.correlation_backward_fused(ad, bd, fdirect, gbuf, 8, SLOPE, *params)
        _same_bits(x1, f1, what + " AUTO (C ABI) grad_input1")
        _same_bits(x2, f2, what + " AUTO (C ABI) grad_input2")
        q1, q2 = torch.empty(0, dtype=dtype, device=dev), torch.empty(0, dtype=dtype, device=dev)
        correlation_cuda.backward_fused(ad, bd, fdirect, gbuf, 8, SLOPE, q1, q2, *params)
        _same_bits(q1, f1, what + " correlation_cuda.backward_fused grad_input1")
        _same_bits(q2, f2, what + " correlation_cuda.backward_fused grad_input2")
        ar, br = ad.clone().requires_grad_(True), bd.clone().requires_grad_(True)
        cat = CorrelationLeakyReLUCat(*params, negative_slope=SLOPE)(ar, br, fdirect[:, :8].contiguous())
        cat.backward(gbuf[:, :8 + nOut].contiguous())
        _same_bits(ar.grad, f1, what + " CorrelationLeakyReLUCat grad_input1")
        _same_bits(br.grad, f2, what + " CorrelationLeakyReLUCat grad_input2")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "md%d-%s" % (c[0], "x".join(map(str, c[1]))))
def test_dense_bits_and_brackets(dev, case, dtype):
    """1. and 2.: forward, fused forward and both gradients equal FN2_CORR_DIRECT bit for bit through every door, and lie in the
    float64 brackets of its documented bounds."""
    md, shape = case
    for fam in _families(shape, dtype):
        ad, bd, fdirect = _forward_case(dev, md, shape, dtype, fam)
        _backward_case(dev, md, shape, dtype, fam, ad, bd, fdirect)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_many_small_items_cross_the_auto_gate(dev, dtype):
    """48 items of 6 x 7 x 37 are 192 workgroups: AUTO's forward is the tiled kernel here, on a shape with leftover channels, a
    ragged last tile row, an odd width (element stores) and an odd slice stride in the fused call -- what the debug variant,
    which has no fused form, cannot reach on the small shapes above."""
    md, shape = 4, (48, 6, 7, 37)
    for fam in ((1, 9) if dtype == F32 else (1, 3)):
        ad, bd, fdirect = _forward_case(dev, md, shape, dtype, fam)
        _backward_case(dev, md, shape, dtype, fam, ad, bd, fdirect)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", MISALIGNED, ids=lambda s: "x".join(map(str, s)))
def test_dense_element_aligned_views(dev, shape, dtype):
    """Inputs, gradOutput and the C ABI's outputs start one element past a 16-byte boundary: the kernels take element-aligned
    pointers.  Every door and the brackets, as for the aligned cases.  The 13-pixel rows rule the forward's pair stores out by the
    width; the 14-pixel rows leave only the pointer to rule them out."""
    for fam in _families(shape, dtype):
        ad, bd, fdirect = _forward_case(dev, 4, shape, dtype, fam, off=1)
        _backward_case(dev, 4, shape, dtype, fam, ad, bd, fdirect, off=1)


def test_dense_debug_variant_names_the_kernel(dev):
    """3.: the debug variant runs inside the domain (before the dense kernels existed the profiling ranges swallowed the value and
    answered FN2_EUNSUPPORTED there) and declines, before anything is launched, outside it; AUTO is then what it was."""
    import fn2_capi
    shape = (2, 8, 10, 12)
    B, C, H, W = shape
    a, b = R.family_inputs(1, shape, seed=3)
    ad, bd = a.to(dev), b.to(dev)
    V = fn2_capi.FN2_DEBUG_CORR_DENSE
    for md in (1, 2, 3, 4):
        for dtype in DTYPES:
            x, y = ad.to(dtype), bd.to(dtype)
            p = _params(md)
            out = fn2_capi.correlation_forward(x, y, *p, algo=V, out=_nan((B,) + L.out_shape(H, W, *p), dtype, dev))
            assert not torch.isnan(out).any()
            g1, g2 = fn2_capi.correlation_backward(x, y, torch.ones_like(out), *p, algo=V,
                                                   out=(_nan(shape, dtype, dev), _nan(shape, dtype, dev)))
            assert not (torch.isnan(g1).any() or torch.isnan(g2).any())
    outside = [((20, 1, 20, 1, 2), F32), ((3, 3, 4, 1, 1), F32), ((4, 1, 4, 2, 1), F32), ((2, 1, 4, 1, 1), F32),
               ((5, 1, 5, 1, 1), F32), ((4, 1, 4, 1, 1), torch.float64)]
    for p, dtype in outside:
        x, y = ad.to(dtype), bd.to(dtype)
        oshape = (B,) + L.out_shape(H, W, *p)
        with pytest.raises(RuntimeError, match=EUNSUPPORTED):
            fn2_capi.correlation_forward(x, y, *p, algo=V, out=_nan(oshape, dtype, dev))
        direct = fn2_capi.correlation_forward(x, y, *p, algo=fn2_capi.FN2_CORR_DIRECT, out=_nan(oshape, dtype, dev))
        auto = fn2_capi.correlation_forward(x, y, *p, out=_nan(oshape, dtype, dev))
        assert not torch.isnan(auto).any()
        if p[4] == 1:    # no other kernel takes these: AUTO is the general kernel
            assert torch.equal(auto, direct), (p, dtype)
        else:
            assert torch.allclose(auto, direct, rtol=1e-4, atol=1e-5), (p, dtype)
        gd = torch.ones(oshape, dtype=dtype, device=dev)
        with pytest.raises(RuntimeError, match=EUNSUPPORTED):
            fn2_capi.correlation_backward(x, y, gd, *p, algo=V)
        if p[3] == 1:    # the backward is defined for stride1 = 1 only
            e1, e2 = fn2_capi.correlation_backward(x, y, gd, *p, algo=fn2_capi.FN2_CORR_DIRECT)
            g1, g2 = fn2_capi.correlation_backward(x, y, gd, *p)
            if p[4] == 1:
                assert torch.equal(g1, e1) and torch.equal(g2, e2), (p, dtype)
            else:
                assert torch.allclose(g1, e1, rtol=1e-4, atol=1e-5) and torch.allclose(g2, e2, rtol=1e-4, atol=1e-5), (p, dtype)


def _windows(fn_auto, fn_direct, calls=20, windows=5):
    """HIP-event times (ms per call) of alternating windows of `calls` calls, after a warm-up."""
    for _ in range(5):
        fn_auto(); fn_direct()
    torch.cuda.synchronize()
    ta, td = [], []
    for _ in range(windows):
        for fn, ts in ((fn_auto, ta), (fn_direct, td)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / calls)
    return ta, td


@pytest.mark.parametrize("case", [((8, 32, 96, 128), F32), ((8, 64, 48, 64), F32), ((8, 32, 96, 128), F16)],
                         ids=["f32-8x32x96x128", "f32-8x64x48x64", "half-8x32x96x128"])
def test_dense_auto_is_the_tiled_kernel(dev, case):
    """4.: bits cannot tell the two kernels apart, a time can: the slowest AUTO window is faster than the fastest FN2_CORR_DIRECT
    window, forward and backward (the bar DESIGN.md 4.8a uses).  It fails while AUTO still runs the general kernel."""
    import statistics

    import fn2_capi
    shape, dtype = case
    params = _params(4)
    B, C, H, W = shape
    a, b = L.family_inputs(1, shape, dtype, seed=11)
    ad, bd = a.to(dev), b.to(dev)
    out = torch.empty((B,) + L.out_shape(H, W, *params), dtype=dtype, device=dev)
    gd = L.grad_output("normal", tuple(out.shape), dtype, seed=12).to(dev)
    g = (torch.empty_like(ad), torch.empty_like(bd))
    runs = {
        "forward": (lambda: fn2_capi.correlation_forward(ad, bd, *params, out=out),
                    lambda: fn2_capi.correlation_forward(ad, bd, *params, algo=fn2_capi.FN2_CORR_DIRECT, out=out)),
        "backward": (lambda: fn2_capi.correlation_backward(ad, bd, gd, *params, out=g),
                     lambda: fn2_capi.correlation_backward(ad, bd, gd, *params, algo=fn2_capi.FN2_CORR_DIRECT, out=g)),
    }
    for name, (fa, fd) in runs.items():
        ta, td = _windows(fa, fd)
        print(f"  {name} {shape} {dtype}: AUTO median {statistics.median(ta) * 1e3:.1f} us (max {max(ta) * 1e3:.1f}), "
              f"FN2_CORR_DIRECT median {statistics.median(td) * 1e3:.1f} us (min {min(td) * 1e3:.1f})")
        assert max(ta) < min(td), (name, shape, dtype, ta, td)


class _PwcBlock(torch.nn.Module):
    """conv -> Correlation(4, 1, 4, 1, 1) -> LeakyReLU -> cat with the features, as PWC-Net's decoder input is written."""

    def __init__(self, fused):
        super().__init__()
        from networks.correlation_package.correlation import Correlation, CorrelationLeakyReLUCat
        self.conv = torch.nn.Conv2d(16, 32, 3, 1, 1)
        self.fused = fused
        self.corr = Correlation(pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=1, corr_multiply=1)
        self.corr_cat = CorrelationLeakyReLUCat(4, 1, 4, 1, 1, negative_slope=0.1)
        self.act = torch.nn.LeakyReLU(0.1)

    def forward(self, x1, x2):
        a, b = self.conv(x1), self.conv(x2)
        a.retain_grad(); b.retain_grad()
        self.seen = (a, b)
        if self.fused:
            return self.corr_cat(a, b, a)
        return torch.cat((a, self.act(self.corr(a, b))), 1)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "bf16-autocast"])
def test_dense_pwc_style_block(dev, autocast):
    """5.: forward and backward run, the dtypes are as expected, fused == unfused bit for bit."""
    res = {}
    for fused in (False, True):
        torch.manual_seed(0)
        net = _PwcBlock(fused).to(dev)
        x1, x2 = torch.randn(2, 16, 24, 40, device=dev), torch.randn(2, 16, 24, 40, device=dev)
        with torch.autocast("cuda", dtype=BF16, enabled=autocast):
            y = net(x1, x2)
            loss = y.float().square().mean()
        loss.backward()
        a, b = net.seen
        want = BF16 if autocast else F32
        assert y.dtype == want and tuple(y.shape) == (2, 32 + 81, 24, 40)
        assert a.grad.dtype == want and b.grad.dtype == want
        assert bool(torch.isfinite(y).all() and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all())
        assert bool(torch.isfinite(net.conv.weight.grad).all())
        res[fused] = (y.detach(), a.grad, b.grad)
    for u, f, name in zip(res[False], res[True], ("output", "grad of in1", "grad of in2")):
        assert torch.equal(_bits(u), _bits(f)), f"fused and unfused {name} differ"
