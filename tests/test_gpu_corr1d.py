"""Correlation1d on the GPU (csrc/correlation_1d.hip through libflownet2_hip_ext.so, correlation1d_cuda and the Python layer).

1. the general kernel is the 2-D general kernel's centre row (pad == md): forward bit for bit, backward as numbers;
2. the general kernel lies in the float64 brackets of the header's bounds, non-finite exactly where a term is not finite, on
   the parameters the 2-D layer cannot express (pad != md, one-sided searches, stride2 = 3);
3. the tiled kernels (FN2X_CORR1D_TILED) have the general kernel's bits, forward and both gradients;
4. every door (AUTO at the C ABI, the pybind module, the autograd Function and Module, another stream) gives those bits, and
   gradcheck passes on double;
5. the same above the forward's AUTO gate;  6. a timing tells that AUTO's forward is the tiled kernel there;
7. the layer beats the PyTorch composition a user would write without it.

Every output is pre-filled with NaN (an unwritten element shows) and sits inside a larger allocation filled with a sentinel that
must be untouched afterwards.  Elements that are NaN in the general kernel's result are compared for NaN-ness only; they may be
at most 5 % of a tensor (a condition on the inputs: family 9 is run only on shapes where its three non-finite operands, nOut
elements each, stay below that)."""
import statistics

import numpy as np
import pytest
import torch

import corr1d_ref as R1
import corr_contract_ref as R
import lowp_ref as L

pytestmark = pytest.mark.gpu

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
NAN_LIMIT = 0.05
SENTINEL = -7777.0
GUARD = 64   # elements on each side of an output; a multiple of 16 bytes for every type

AUTO, GENERAL, TILED = 0, 1, 2
BIG = (8, 32, 96, 128)   # md 40, two-sided: nOut = 81 and 8 x 4 x 24 = 768 tiles of 32 x 4 pixels -- AUTO's forward is the tiled kernel


# ------------------------------------------------------------------ helpers
def _guarded(shape, dtype, dev, off=0):
    """(view, whole): a NaN-filled tensor of `shape` inside a sentinel-filled allocation; off = 1 starts it one element past a
    16-byte boundary."""
    n = int(np.prod(shape))
    whole = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=dtype, device=dev)
    view = whole[GUARD + off:GUARD + off + n].view(shape)
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == (off * whole.element_size()) % 16
    return view, whole


def _untouched(whole, view, what):
    n, lo = view.numel(), view.storage_offset()
    assert bool((whole[:lo] == SENTINEL).all()) and bool((whole[lo + n:] == SENTINEL).all()), f"{what}: wrote outside its output"


def _place(t, dev, off=0):
    if not off:
        return t.to(dev)
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    v = flat[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * t.element_size()
    return v


def _bits(t):
    return t.contiguous().view({F32: torch.int32, F64: torch.int64}.get(t.dtype, torch.int16))


def _same_bits(got, want, what):
    """got == want bit for bit, except that where the general kernel's result is NaN the other must be NaN (any payload)."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = torch.isnan(want)
    frac = float(nan.double().mean()) if nan.numel() else 0.0
    assert frac <= NAN_LIMIT, f"{what}: {frac:.3%} of the general kernel's elements are NaN"
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN elements differ from the general kernel's"
    bad = (_bits(got) != _bits(want)) & ~nan
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ from the general kernel; first at flat index {i}: "
                             f"{float(got.flatten()[i])!r} vs {float(want.flatten()[i])!r}")


def _inputs(fam, shape, dtype, seed):
    if dtype == F32:
        return R.family_inputs(fam, shape, seed)
    if dtype == F64:
        a, b = R.family_inputs(fam, shape, seed)
        return a.double(), b.double()
    return L.family_inputs(fam, shape, dtype, seed)


def _gout(kind, shape, dtype, seed):
    if dtype in (F32, F64):
        return R.grad_output(kind, shape, seed).to(dtype)
    return L.grad_output(kind, shape, dtype, seed)


def _fwd(ad, bd, prm, algo, off=0, what="forward"):
    import fn2_capi
    B, C, H, W = ad.shape
    oshape = (B,) + fn2_capi.correlation1d_output_shape(H, W, *prm)
    out, whole = _guarded(oshape, ad.dtype, ad.device, off)
    fn2_capi.correlation1d_forward(ad, bd, *prm, algo=algo, out=out)
    _untouched(whole, out, what)
    return out


def _bwd(ad, bd, gd, prm, algo, off=0, what="backward"):
    import fn2_capi
    (g1, w1), (g2, w2) = _guarded(ad.shape, ad.dtype, ad.device, off), _guarded(ad.shape, ad.dtype, ad.device, off)
    fn2_capi.correlation1d_backward(ad, bd, gd, *prm, algo=algo, out=(g1, g2))
    _untouched(w1, g1, what + " grad_input1")
    _untouched(w2, g2, what + " grad_input2")
    return g1, g2


def _written(t, ad, bd, what):
    if not (torch.isnan(ad).any() or torch.isnan(bd).any() or torch.isinf(ad).any() or torch.isinf(bd).any()):
        assert not torch.isnan(t).any(), f"{what}: elements left unwritten"


# ------------------------------------------------------------------ 1. the general kernel is the 2-D general kernel's centre row
@pytest.mark.parametrize("dtype", [F32, F16, BF16, F64], ids=["f32", "half", "bf16", "f64"])
@pytest.mark.parametrize("shape", [(2, 7, 5, 31), (1, 34, 3, 100)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", [(4, 1, 1), (40, 1, 1), (6, 1, 2), (5, 2, 1)], ids=lambda c: "md%d-s1_%d-s2_%d" % c)
def test_general_is_the_centre_row_of_the_2d_general_kernel(dev, case, shape, dtype):
    import fn2_capi
    md, s1, s2 = case
    dr = md // s2
    D = 2 * dr + 1
    rows = slice(dr * D, (dr + 1) * D)
    fams = {F32: (1, 2, 9), F64: (1, 2, 9)}.get(dtype, (1, 3))
    for fam in fams:
        what = f"md {md} s1 {s1} s2 {s2} {shape} {dtype} family {fam}"
        a, b = _inputs(fam, shape, dtype, seed=md + sum(shape))
        ad, bd = a.to(dev), b.to(dev)
        full = fn2_capi.correlation_forward(ad, bd, md, 1, md, s1, s2, algo=fn2_capi.FN2_CORR_DIRECT)
        for sd, sl in ((0, slice(0, D)), (-1, slice(0, dr + 1)), (1, slice(dr, D))):
            out = _fwd(ad, bd, (md, md, s1, s2, sd), GENERAL, what=what)
            _written(out, ad, bd, what)
            want = full[:, rows][:, sl].contiguous()
            assert torch.equal(torch.isnan(out), torch.isnan(want)), what
            assert torch.equal(_bits(out)[~torch.isnan(want)], _bits(want)[~torch.isnan(want)]), f"{what} sd {sd}: forward bits differ"
        if s1 != 1 or fam == 9:
            continue   # the backward: stride1 = 1, finite inputs
        for kind in ("normal", "window"):
            oshape = (shape[0], D) + tuple(full.shape[2:])
            gd = _gout(kind, oshape, dtype, seed=fam + md).to(dev)
            g2d = torch.zeros_like(full)
            g2d[:, rows] = gd
            e1, e2 = fn2_capi.correlation_backward(ad, bd, g2d, md, 1, md, s1, s2, algo=fn2_capi.FN2_CORR_DIRECT)
            g1, g2 = _bwd(ad, bd, gd, (md, md, s1, s2, 0), GENERAL, what=what)
            assert torch.equal(g1, e1) and torch.equal(g2, e2), f"{what} gradOutput {kind}: gradients differ from the 2-D layer's"


# ------------------------------------------------------------------ 2. the general kernel inside the float64 brackets
def _check_bracket(got, ref, absr, bad, delta, dtype, what):
    dev = got.device
    ref, absr, bad = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (ref, absr, bad))
    fin = ~bad
    assert torch.equal(torch.isfinite(got), fin), f"{what}: non-finite outputs differ from the float64 reference's"
    d = delta(ref, absr)
    if dtype == F64:   # (the backward of double tensors: compared in float64 directly, there is nothing to round to)
        err = (got[fin] - ref[fin]).abs()
        assert bool((err <= d[fin]).all()), f"{what}: {float((err / d[fin].clamp(min=1e-300)).max()):.3g} x the bound"
        return
    lo, hi = L.bracket(ref[fin], d[fin], F32 if dtype == "f64fwd" else dtype)
    L.check_bracket(got[fin].float() if dtype == "f64fwd" else got[fin], lo, hi, what)


BRACKET_CASES = [  # pad, md, s1, s2, sd
    (2, 5, 1, 1, 0), (0, 3, 1, 1, 0), (4, 4, 1, 1, -1), (4, 4, 1, 1, 1), (7, 7, 1, 3, 0), (2, 5, 1, 1, -1), (1, 6, 1, 2, 1), (3, 5, 2, 1, 0)]


@pytest.mark.parametrize("dtype", [F32, F16, BF16, F64], ids=["f32", "half", "bf16", "f64"])
@pytest.mark.parametrize("prm", BRACKET_CASES, ids=lambda p: "pad%d-md%d-s1_%d-s2_%d-sd%d" % p)
def test_general_inside_the_float64_brackets(dev, prm, dtype):
    pad, md, s1, s2, sd = prm
    shape = (2, 7, 5, 31)
    B, C, H, W = shape
    nOut = R1.out_shape(H, W, *prm)[0]
    fams = {F32: (1, 2, 8, 9), F64: (1, 9)}.get(dtype, (1, 2, 4))
    fwd_delta = {F32: lambda r, s: R.delta_direct_f32(r, s, C), F64: lambda r, s: R.delta_direct_f32(r, s, C),
                 F16: lambda r, s: L.delta_fwd_direct_half(r, s, C), BF16: lambda r, s: L.delta_fwd(r, s, C)}[dtype]
    bwd_delta = {F32: lambda r, s: R.delta_direct_bwd_f32(r, s, nOut), F64: lambda r, s: R.delta_direct_bwd_f64(r, s, nOut)}.get(
        dtype, lambda r, s: nOut * L.U23 * s + L.U23 * r.abs())
    for fam in fams:
        what = f"{prm} {dtype} family {fam}"
        a, b = _inputs(fam, shape, dtype, seed=pad + md + s2)
        ad, bd = a.to(dev), b.to(dev)
        out = _fwd(ad, bd, prm, GENERAL, what=what)
        ref, absr, bad = R1.forward(a.double().numpy(), b.double().numpy(), *prm)
        # double tensors: the forward accumulates in float, so its result is an fp32 value inside the fp32 bracket
        _check_bracket(out, ref, absr, bad, fwd_delta, "f64fwd" if dtype == F64 else dtype, what + " forward")
        if s1 != 1:
            continue
        for kind in ("normal", "leaky"):
            g = _gout(kind, tuple(out.shape), dtype, seed=fam + md)
            g1, g2 = _bwd(ad, bd, g.to(dev), prm, GENERAL, what=what)
            res = R1.backward(a.double().numpy(), b.double().numpy(), g.double().numpy(), *prm)
            for got, (r, s, nf), name in ((g1, res[0], "grad_input1"), (g2, res[1], "grad_input2")):
                _check_bracket(got, r, s, nf, bwd_delta, dtype, f"{what} gradOutput {kind} {name}")


# ------------------------------------------------------------------ 3. tiled == general, bit for bit
# (shape, md, single_directions)
TILED_CASES = [((1, 1, 1, 1), 4, (-1, 0, 1)), ((1, 5, 1, 33), 40, (-1, 0, 1)), ((2, 7, 5, 31), 4, (-1, 0, 1)), ((1, 34, 9, 130), 40, (-1, 0, 1)),
               ((2, 6, 13, 64), 7, (-1, 0, 1)), ((1, 196, 3, 8), 3, (-1, 0, 1)), ((1, 4, 3, 100), 80, (-1, 1)), ((3, 9, 17, 32), 1, (-1, 0, 1))]
MISALIGNED = [((2, 7, 5, 31), 4), ((2, 6, 13, 64), 7)]


def _family9_fits(shape, nOut):
    """Family 9 holds at most three non-finite operands; each reaches at most nOut elements of one row (forward) or of one
    channel's row (backward)."""
    B, C, H, W = shape
    return 3 * nOut <= NAN_LIMIT * B * nOut * H * W and 3 * nOut <= NAN_LIMIT * B * C * H * W


def _families(shape, dtype, nOut):
    fams = list(R.FAMILIES) if dtype == F32 else [1, 2, 3, 4, 5]
    return [f for f in fams if f != 9 or _family9_fits(shape, nOut)]


def _tiled_case(dev, shape, md, sd, dtype, fams, off=0, algos=(TILED,)):
    prm = (md, md, 1, 1, sd)
    B, C, H, W = shape
    nOut = R1.out_shape(H, W, *prm)[0]
    for fam in fams:
        what = f"{shape} md {md} sd {sd} {dtype} family {fam}"
        a, b = _inputs(fam, shape, dtype, seed=sum(shape) + md)
        ad, bd = _place(a, dev, off), _place(b, dev, off)
        want = _fwd(ad, bd, prm, GENERAL, off, what)
        _written(want, ad, bd, what + " general forward")
        for algo in algos:
            _same_bits(_fwd(ad, bd, prm, algo, off, what), want, f"{what} forward algo {algo}")
        for kind in ("normal", "leaky", "window"):
            gd = _place(_gout(kind, (B, nOut, H, W), dtype, seed=fam + md), dev, off)
            w1, w2 = _bwd(ad, bd, gd, prm, GENERAL, off, what)
            _written(w1, ad, bd, what + " general backward")
            for algo in algos:
                g1, g2 = _bwd(ad, bd, gd, prm, algo, off, what)
                _same_bits(g1, w1, f"{what} gradOutput {kind} grad_input1 algo {algo}")
                _same_bits(g2, w2, f"{what} gradOutput {kind} grad_input2 algo {algo}")


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "half", "bf16"])
@pytest.mark.parametrize("case", TILED_CASES, ids=lambda c: "%s-md%d" % ("x".join(map(str, c[0])), c[1]))
def test_tiled_has_the_general_kernels_bits(dev, case, dtype):
    shape, md, sds = case
    for sd in sds:
        nOut = R1.out_shape(shape[2], shape[3], md, md, 1, 1, sd)[0]
        _tiled_case(dev, shape, md, sd, dtype, _families(shape, dtype, nOut))


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "half", "bf16"])
@pytest.mark.parametrize("case", MISALIGNED, ids=lambda c: "%s-md%d" % ("x".join(map(str, c[0])), c[1]))
def test_tiled_on_element_aligned_views(dev, case, dtype):
    """Inputs, gradOutput and outputs start one element past a 16-byte boundary: the kernels take element-aligned pointers (the
    64-pixel rows leave only the pointer to rule the forward's pair stores out)."""
    shape, md = case
    for sd in (-1, 0, 1):
        _tiled_case(dev, shape, md, sd, dtype, (1, 9) if dtype == F32 else (1, 3), off=1)


# ------------------------------------------------------------------ 4. every door
@pytest.mark.parametrize("dtype", [F32, F16, BF16, F64], ids=["f32", "half", "bf16", "f64"])
@pytest.mark.parametrize("sd", [-1, 0, 1])
def test_every_door_gives_the_general_kernels_bits(dev, sd, dtype):
    import correlation1d_cuda
    import fn2_capi
    from networks.correlation_package import Correlation1d, Correlation1dFunction
    shape, md = (2, 7, 5, 31), 4
    prm = (md, md, 1, 1, sd)
    a, b = _inputs(1, shape, dtype, seed=5)
    ad, bd = a.to(dev), b.to(dev)
    want = _fwd(ad, bd, prm, GENERAL)
    gd = _gout("normal", tuple(want.shape), dtype, seed=6).to(dev)
    w1, w2 = _bwd(ad, bd, gd, prm, GENERAL)
    what = f"sd {sd} {dtype}"
    _same_bits(_fwd(ad, bd, prm, AUTO), want, what + " AUTO (C ABI)")
    for g, w in zip(_bwd(ad, bd, gd, prm, AUTO), (w1, w2)):
        _same_bits(g, w, what + " AUTO (C ABI) backward")
    # caller-provided tensors, resized in place
    o = torch.empty(0, dtype=dtype, device=dev)
    correlation1d_cuda.forward(ad, bd, o, *prm)
    _same_bits(o, want, what + " correlation1d_cuda.forward")
    p1, p2 = torch.empty(0, dtype=dtype, device=dev), torch.empty(0, dtype=dtype, device=dev)
    correlation1d_cuda.backward(ad, bd, gd, p1, p2, *prm)
    _same_bits(p1, w1, what + " correlation1d_cuda.backward")
    _same_bits(p2, w2, what + " correlation1d_cuda.backward")
    _same_bits(correlation1d_cuda.forward_alloc(ad, bd, *prm), want, what + " forward_alloc")
    for g, w in zip(correlation1d_cuda.backward_alloc(ad, bd, gd, *prm), (w1, w2)):
        _same_bits(g, w, what + " backward_alloc")
    # the autograd Function and the Module
    for name, fn in (("Correlation1dFunction.apply", lambda x, y: Correlation1dFunction.apply(x, y, *prm)), ("Correlation1d", Correlation1d(*prm))):
        ar, br = ad.clone().requires_grad_(True), bd.clone().requires_grad_(True)
        out = fn(ar, br)
        _same_bits(out.detach(), want, f"{what} {name}")
        out.backward(gd)
        _same_bits(ar.grad, w1, f"{what} {name} grad_input1")
        _same_bits(br.grad, w2, f"{what} {name} grad_input2")
    # a second differentiation raises
    ar, br = ad.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(Correlation1d(*prm)(ar, br).float().sum(), ar, create_graph=False)
    assert g1.shape == ar.shape
    if dtype == F32:
        out = Correlation1d(*prm)(ar, br)
        gr = gd.clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match="not differentiable a second time"):
            torch.autograd.grad(out, ar, gr, create_graph=True)
    # a non-default stream
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        so = fn2_capi.correlation1d_forward(ad, bd, *prm)
        s1, s2 = fn2_capi.correlation1d_backward(ad, bd, gd, *prm)
        mo = Correlation1d(*prm)(ad, bd)
    s.synchronize()
    _same_bits(so, want, what + " forward on another stream")
    _same_bits(mo, want, what + " module on another stream")
    _same_bits(s1, w1, what + " backward on another stream")
    _same_bits(s2, w2, what + " backward on another stream")


@pytest.mark.parametrize("sd", [-1, 0, 1])
def test_gradcheck_on_double(dev, sd):
    """torch.autograd.gradcheck with its defaults (eps 1e-6, atol 1e-5, rtol 1e-3).  The forward of double tensors accumulates in
    float (the general 2-D kernel's contract), so central differences see its rounding: about 2^-24 |out| / eps.  Inputs of
    magnitude 2^-8 keep that below 1e-5 (|out| <= 9 * 2^-16 at three sigma: 8e-12 / 2e-6 = 4e-6) while the gradients, about
    2^-8 / 3, stay a hundred times above the tolerance."""
    from networks.correlation_package import Correlation1dFunction
    g = torch.Generator().manual_seed(7 + sd)
    a = (torch.randn(1, 3, 3, 9, generator=g, dtype=F64) * 2.0 ** -8).to(dev).requires_grad_()
    b = (torch.randn(1, 3, 3, 9, generator=g, dtype=F64) * 2.0 ** -8).to(dev).requires_grad_()
    assert torch.autograd.gradcheck(lambda x, y: Correlation1dFunction.apply(x, y, 2, 2, 1, 1, sd), (a, b))


# ------------------------------------------------------------------ 5. above the forward's AUTO gate
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "half", "bf16"])
def test_above_the_gate_auto_tiled_and_general_agree(dev, dtype):
    _tiled_case(dev, BIG, 40, 0, dtype, (1, 9) if dtype == F32 else (1,), algos=(TILED, AUTO))


# ------------------------------------------------------------------ 6. which kernel ran
def _windows(fns, calls=10, windows=5):
    """HIP-event times (ms per call) of alternating windows of `calls` calls of each function, after a warm-up."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(windows):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / calls)
    return ts


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "half"])
def test_auto_forward_above_the_gate_is_the_tiled_kernel(dev, dtype):
    """Bits cannot tell the kernels apart, a time can: AUTO's median lies inside the spread of FN2X_CORR1D_TILED's windows (10 %
    each way), and where the tiled and the general kernel are clearly apart (no overlap of their windows) every AUTO window is
    on the tiled side."""
    import fn2_capi
    prm = (40, 40, 1, 1, 0)
    a, b = L.family_inputs(1, BIG, dtype, seed=11)
    ad, bd = a.to(dev), b.to(dev)
    out = torch.empty((BIG[0], 81) + BIG[2:], dtype=dtype, device=dev)
    ta, tt, tg = _windows([lambda algo=algo: fn2_capi.correlation1d_forward(ad, bd, *prm, algo=algo, out=out) for algo in (AUTO, TILED, GENERAL)])
    ma, mt, mg = (statistics.median(t) for t in (ta, tt, tg))
    print(f"  forward {BIG} md 40 {dtype}: AUTO {ma * 1e3:.1f} us, tiled {mt * 1e3:.1f} us [{min(tt) * 1e3:.1f}, {max(tt) * 1e3:.1f}], "
          f"general {mg * 1e3:.1f} us [{min(tg) * 1e3:.1f}, {max(tg) * 1e3:.1f}]")
    assert 0.9 * min(tt) <= ma <= 1.1 * max(tt), (ta, tt, tg)
    if max(tt) < min(tg):
        assert max(ta) < min(tg), (ta, tt, tg)
    elif max(tg) < min(tt):
        assert min(ta) > max(tg), (ta, tt, tg)


# ------------------------------------------------------------------ 7. worth having
def _composition(a, b, md):
    """What a user writes without the layer: pad in2, one shifted product per displacement, mean over the channels, stack."""
    W = a.shape[-1]
    bp = torch.nn.functional.pad(b, (md, md))
    return torch.stack([(a * bp[..., j:j + W]).mean(1) for j in range(2 * md + 1)], 1)


def test_layer_beats_the_pytorch_composition(dev):
    """(2, 64, 48, 96), md 40, fp32, forward + backward, medians of alternating windows.  Only "faster" is asserted: the
    composition's forward alone reads both operands once per displacement, 81 x the layer's input traffic, so even a layer at a
    tenth of the achievable bandwidth wins.  The ratio is printed, not asserted."""
    from networks.correlation_package import Correlation1d
    shape, md = (2, 64, 48, 96), 40
    a, b = R.family_inputs(1, shape, seed=3)
    ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    layer = Correlation1d(md, md, 1, 1, 0)
    gd = R.grad_output("normal", (2, 81, 48, 96), seed=4).to(dev)
    with torch.no_grad():
        ref, out = _composition(ad, bd, md), layer(ad, bd)
    # (a sanity check that the two are the same function, not a precision pin: tests 1 - 3 are those)
    assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), "the composition is the same function"

    def run(fn):
        ad.grad = bd.grad = None
        fn(ad, bd).backward(gd)

    tl, tc = _windows([lambda: run(layer), lambda: run(lambda x, y: _composition(x, y, md))], calls=3, windows=5)
    ml, mc = statistics.median(tl), statistics.median(tc)
    print(f"  Correlation1d {ml * 1e3:.1f} us, composition {mc * 1e3:.1f} us per forward + backward: {mc / ml:.1f} x")
    assert ml < mc, (tl, tc)
