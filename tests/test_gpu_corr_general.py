"""Correlation off FlowNetC's configuration on the GPU, element by element against float64.

The parameter-general kernels (csrc/correlation_direct.hip: the bit reference of the dense and 1-D tiled kernels) on the grid of
tests/corr_general_ref.py -- pad below, at and above md, kernel_size 1 / 2 / 3 / 5, md 0, md % s2 != 0, stride1 2 and 3, single
pixels and rows -- in all four dtypes, forward (a) and backward (b), with non-finite operands (c), through the fused entry points
(d), past the backward's grid cap (e) and through the autograd Module (f); and the fp32 matrix kernels (csrc/correlation_mfma.hip,
correlation_mfma_bwd.hip) at every radius they accept (g), where the test restates the launchers' conditions to say which kernel
it reached.  tests/test_corr_general_host.py shows on the CPU that a correct kernel meets these bounds on these inputs and that
a kernel with an indexing mistake does not.

Every output is prefilled with NaN inside a sentinel-guarded allocation (tests/test_gpu_corr1d.py); every check prints its worst
err / delta, and the last test reports the largest per (quantity, dtype, kernel): measured values, not assertions."""
import numpy as np
import pytest
import torch

import corr_contract_ref as R
import corr_general_ref as G
import lowp_ref as L
from test_gpu_corr1d import _bits, _guarded, _untouched

pytestmark = pytest.mark.gpu

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
DTYPES = [F32, F64, F16, BF16]
DTYPE_IDS = ["f32", "f64", "half", "bf16"]
NAME = dict(zip(DTYPES, DTYPE_IDS))
EUNSUPPORTED = r"code -4"
SLOPE = 0.1
WORST = {}   # (quantity, dtype, kernel) -> the largest err / delta seen in this run


# ------------------------------------------------------------------ helpers
def _families(dtype):
    return (1, 2, 3, 5, 7, 8) if dtype in (F32, F64) else (1, 2, 3, 4, 5)


def _inputs(fam, shape, dtype, seed):
    if dtype in (F32, F64):
        a, b = R.family_inputs(fam, shape, seed)
        return a.to(dtype), b.to(dtype)
    return L.family_inputs(fam, shape, dtype, seed)


def _gout(kind, shape, dtype, seed):
    if dtype in (F32, F64):
        return R.grad_output(kind, shape, seed).to(dtype)
    return L.grad_output(kind, shape, dtype, seed)


def _oshape(shape, params):
    B, C, H, W = shape
    return (B,) + L.out_shape(H, W, *params)


def _fwd(ad, bd, params, algo, what):
    import fn2_capi
    out, whole = _guarded(_oshape(ad.shape, params), ad.dtype, ad.device)
    fn2_capi.correlation_forward(ad, bd, *params, algo=algo, out=out)
    _untouched(whole, out, what)
    return out


def _fwd_declines(ad, bd, params, algo, what):
    import fn2_capi
    out, whole = _guarded(_oshape(ad.shape, params), ad.dtype, ad.device)
    with pytest.raises(RuntimeError, match=EUNSUPPORTED):
        fn2_capi.correlation_forward(ad, bd, *params, algo=algo, out=out)
    _untouched(whole, out, what)
    assert bool(torch.isnan(out).all()), f"{what}: a declined call wrote to its output"


def _bwd(ad, bd, gd, params, algo, what):
    import fn2_capi
    (g1, w1), (g2, w2) = _guarded(ad.shape, ad.dtype, ad.device), _guarded(ad.shape, ad.dtype, ad.device)
    fn2_capi.correlation_backward(ad, bd, gd, *params, algo=algo, out=(g1, g2))
    _untouched(w1, g1, what + " grad_input1")
    _untouched(w2, g2, what + " grad_input2")
    return g1, g2


def _bwd_declines(ad, bd, gd, params, algo, what):
    import fn2_capi
    (g1, w1), (g2, w2) = _guarded(ad.shape, ad.dtype, ad.device), _guarded(ad.shape, ad.dtype, ad.device)
    with pytest.raises(RuntimeError, match=EUNSUPPORTED):
        fn2_capi.correlation_backward(ad, bd, gd, *params, algo=algo, out=(g1, g2))
    _untouched(w1, g1, what)
    _untouched(w2, g2, what)
    assert bool(torch.isnan(g1).all() and torch.isnan(g2).all()), f"{what}: a declined call wrote to its gradients"


def _same(x, y, what):
    assert x.shape == y.shape and x.dtype == y.dtype, what
    nan = torch.isnan(y)
    assert torch.equal(torch.isnan(x), nan) and torch.equal(_bits(x)[~nan], _bits(y)[~nan]), f"{what}: bits differ"


def _half_ulp(ref, dtype):
    """Half of the spacing of `dtype` at |ref|: what the one rounding to a 16-bit type adds to the fp32 bound (for the report)."""
    mant, emin = (10, -14) if dtype == F16 else (7, -126)
    e = (torch.frexp(ref.abs().clamp(min=1e-300))[1] - 1).clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref), e - mant - 1)


def _check(got, ref, delta, what, key, post=None, nonfinite=None):
    """Every element of `got` in the bracket of ref +- delta for its type (double: compared in double, nothing to round to),
    non-finite exactly where `nonfinite` says (default: nowhere); prints and records the worst err / delta (for the 16-bit
    types: relative to delta plus half a unit of the type, the final rounding)."""
    dtype = got.dtype
    fin = torch.ones_like(ref, dtype=torch.bool) if nonfinite is None else ~nonfinite
    assert torch.equal(torch.isfinite(got), fin), f"{what}: non-finite outputs differ from the expected ones"
    ref, delta, g = ref[fin], delta[fin], got[fin]
    if dtype == F64:
        assert post is None
        lo, hi = ref - delta, ref + delta
    else:
        lo, hi = L.bracket(ref, delta, dtype, post=post)
    L.check_bracket(g, lo, hi, what)
    target = ref if post is None else post(ref.float()).double()
    room = delta + (_half_ulp(target, dtype) if dtype in (F16, BF16) else 0.0)
    ratio = float(((g.double() - target).abs() / room.clamp(min=1e-300)).max()) if g.numel() else 0.0
    print(f"  {what}: worst err/delta {ratio:.3g}")
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return ratio


def _fwd_delta(dtype, ref, absr, C, k):
    if dtype in (F32, F64):    # the double kernel accumulates in float: the fp32 bound, compared in double
        return R.delta_direct_f32(ref, absr, C, k)
    return L.delta_fwd_direct_half(ref, absr, C, k) if dtype == F16 else L.delta_fwd(ref, absr, C, k)


def _bwd_delta(dtype, ref, absr, params):
    pad, k, md, s1, s2 = params
    if dtype == F32:
        return R.delta_direct_bwd_f32(ref, absr, L.n_bwd(md, s2, k))
    if dtype == F64:
        return R.delta_direct_bwd_f64(ref, absr, L.n_bwd(md, s2, k))
    return L.delta_bwd(ref, absr, md, s2, k)


def _leaky(dtype):
    return L.leaky_general(SLOPE, dtype)


# ------------------------------------------------------------------ a. forward on the whole grid
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", G.GRID, ids=G.case_id)
def test_general_forward(dev, case, dtype):
    import fn2_capi
    params, shape = case
    C, k = shape[1], params[1]
    for fam in _families(dtype):
        what = f"general fwd {G.case_id(case)} {NAME[dtype]} family {fam}"
        a, b = _inputs(fam, shape, dtype, seed=sum(shape) + sum(params))
        ad, bd = a.to(dev), b.to(dev)
        out = _fwd(ad, bd, params, fn2_capi.FN2_CORR_DIRECT, what)
        _same(_fwd(ad, bd, params, fn2_capi.FN2_CORR_AUTO, what + " AUTO"), out, what + " AUTO vs DIRECT")
        for algo in (fn2_capi.FN2_CORR_MFMA_F16X2, fn2_capi.FN2_CORR_MFMA_F32):
            _fwd_declines(ad, bd, params, algo, f"{what} algo {algo}")
        ref = L.corr_fwd64(ad, bd, *params)
        absr = L.corr_fwd64(ad.abs(), bd.abs(), *params)
        _check(out, ref, _fwd_delta(dtype, ref, absr, C, k), what, ("forward", NAME[dtype], "general"))


def test_empty_output_is_einval(dev):
    import fn2_capi
    params, shape = G.EMPTY
    a = torch.zeros(shape, device=dev)
    with pytest.raises(RuntimeError, match=r"code -1"):
        fn2_capi.correlation_forward(a, a, *params)
    assert fn2_capi.lib().fn2_correlation_output_shape(shape[2], shape[3], *params, None, None, None) == -1


# ------------------------------------------------------------------ b. backward on the grid
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", G.GRID, ids=G.case_id)
def test_general_backward(dev, case, dtype):
    import fn2_capi
    params, shape = case
    oshape = _oshape(shape, params)
    if params[3] != 1:   # the backward is defined for stride1 = 1 only: declined in front of any launch
        a, b = _inputs(1, shape, dtype, seed=3)
        gd = _gout("normal", oshape, dtype, seed=4).to(dev)
        for algo in (fn2_capi.FN2_CORR_AUTO, fn2_capi.FN2_CORR_DIRECT):
            _bwd_declines(a.to(dev), b.to(dev), gd, params, algo, f"general bwd {G.case_id(case)} {NAME[dtype]} algo {algo}")
        return
    for fam in _families(dtype):
        a, b = _inputs(fam, shape, dtype, seed=sum(shape) + sum(params))
        ad, bd = a.to(dev), b.to(dev)
        for kind in ("normal", "window") if fam == 1 else ("normal",):
            what = f"general bwd {G.case_id(case)} {NAME[dtype]} family {fam} gradOutput {kind}"
            gd = _gout(kind, oshape, dtype, seed=fam + params[2]).to(dev)
            g1, g2 = _bwd(ad, bd, gd, params, fn2_capi.FN2_CORR_DIRECT, what)
            for g, w in zip(_bwd(ad, bd, gd, params, fn2_capi.FN2_CORR_AUTO, what + " AUTO"), (g1, g2)):
                _same(g, w, what + " AUTO vs DIRECT")
            r1, r2 = L.corr_bwd64(ad, bd, gd, *params)
            ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), gd.abs(), *params)
            _check(g1, r1, _bwd_delta(dtype, r1, ab1, params), what + " grad_input1", ("backward", NAME[dtype], "general"))
            _check(g2, r2, _bwd_delta(dtype, r2, ab2, params), what + " grad_input2", ("backward", NAME[dtype], "general"))


# ------------------------------------------------------------------ c. non-finite operands
@pytest.mark.parametrize("case", [G.GRID[2], G.GRID[3]], ids=G.case_id)
def test_general_nonfinite_operands(dev, case):
    """Family 9 (+inf in in1's top-left corner, nan in in2's bottom-right corner, operands up to 2^20) with one more inf and nan
    at the centre: outputs are non-finite
    exactly where a term has both operands in the image and a non-finite product, and in their brackets elsewhere."""
    import fn2_capi
    params, shape = case
    assert params in ((2, 1, 4, 1, 1), (6, 1, 4, 1, 2))
    C, k = shape[1], params[1]
    what = f"general non-finite {G.case_id(case)}"
    a, b = R.family_inputs(9, shape, seed=sum(shape))
    # family 9 keeps its non-finite operands in the corners, which a layer with pad < md never reads (its outputs are centred on
    # rows md - pad .. H - 1 - (md - pad)): one more of each at the map's centre, so that every output has non-finite elements
    B, H, W = shape[0], shape[2], shape[3]
    a[B - 1, 0, H // 2, W // 2] = -float("inf")
    b[0, C - 1, H // 2, W // 2] = float("nan")
    ad, bd = a.to(dev), b.to(dev)
    assert not bool(torch.isfinite(ad).all()) and not bool(torch.isfinite(bd).all())
    af, bf = R.finite_part(ad.double()), R.finite_part(bd.double())
    nonfin = R.fwd_nonfinite(ad, bd, params)
    assert 0.0 < float(nonfin.double().mean()) < 0.5, "a condition on the input: some, but not most, outputs are non-finite"
    out = _fwd(ad, bd, params, fn2_capi.FN2_CORR_DIRECT, what)
    ref, absr = L.corr_fwd64(af, bf, *params), L.corr_fwd64(af.abs(), bf.abs(), *params)
    _check(out, ref, R.delta_direct_f32(ref, absr, C, k), what + " forward", ("forward", "f32", "general"), nonfinite=nonfin)
    gd = R.grad_output("normal", _oshape(shape, params), seed=9).to(dev)
    nf1, nf2 = R.bwd_nonfinite(ad, bd, gd, params)
    for nf in (nf1, nf2):
        assert 0.0 < float(nf.double().mean()) < 0.5
    g1, g2 = _bwd(ad, bd, gd, params, fn2_capi.FN2_CORR_DIRECT, what)
    r1, r2 = L.corr_bwd64(af, bf, gd, *params)
    ab1, ab2 = L.corr_bwd64(af.abs(), bf.abs(), gd.abs(), *params)
    _check(g1, r1, _bwd_delta(F32, r1, ab1, params), what + " grad_input1", ("backward", "f32", "general"), nonfinite=nf1)
    _check(g2, r2, _bwd_delta(F32, r2, ab2, params), what + " grad_input2", ("backward", "f32", "general"), nonfinite=nf2)


# ------------------------------------------------------------------ d. the fused doors
FUSED = [(((4, 3, 5, 1, 2), (1, 33, 7, 10)), False), (((2, 1, 4, 1, 1), (2, 8, 12, 16)), True)]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "half"])
@pytest.mark.parametrize("case,x4", FUSED, ids=[G.case_id(c) for c, _ in FUSED])
def test_general_fused_doors(dev, case, x4, dtype):
    """fn2_correlation_forward_fused into a buffer with 8 channels in front and 3 behind (a batch stride wider than the volume,
    slope 0.1), and fn2_correlation_backward_fused: the bits of the composition.  The first case's volume is no multiple of four
    elements per item and takes the scalar mask kernel, the second's is and takes mask_slice_f32x4 on float32 tensors."""
    import fn2_capi
    params, shape = case
    B, C, H, W = shape
    k = params[1]
    nOut, oH, oW = L.out_shape(H, W, *params)
    n_item = nOut * oH * oW
    assert (n_item % 4 == 0) == x4 and (not x4 or ((8 + nOut + 3) * oH * oW) % 4 == 0)
    what = f"general fused {G.case_id(case)} {NAME[dtype]}"
    a, b = _inputs(1, shape, dtype, seed=sum(shape))
    ad, bd = a.to(dev), b.to(dev)
    ref, absr = L.corr_fwd64(ad, bd, *params), L.corr_fwd64(ad.abs(), bd.abs(), *params)
    assert float((ref < 0).double().mean()) > 0.2 and float((ref > 0).double().mean()) > 0.2, "both branches of the activation"
    # forward
    buf, whole = _guarded((B, 8 + nOut + 3, oH, oW), dtype, dev)
    g = torch.Generator(device=dev).manual_seed(sum(shape))
    buf[:, :8] = torch.randn((B, 8, oH, oW), generator=g, device=dev).to(dtype)
    buf[:, 8 + nOut:] = torch.randn((B, 3, oH, oW), generator=g, device=dev).to(dtype)
    before = buf.clone()
    fn2_capi.correlation_forward_fused(ad, bd, buf, 8, SLOPE, *params)
    _untouched(whole, buf, what)
    assert torch.equal(_bits(buf[:, :8]), _bits(before[:, :8])) and torch.equal(_bits(buf[:, 8 + nOut:]), _bits(before[:, 8 + nOut:])), \
        f"{what}: the neighbouring channels changed"
    act = buf[:, 8:8 + nOut]
    _check(act, ref, _fwd_delta(dtype, ref, absr, C, k), what + " forward", ("forward fused", NAME[dtype], "general"), post=_leaky(dtype))
    # backward
    gbuf = _gout("normal", tuple(buf.shape), dtype, seed=sum(shape) + 1).to(dev)
    gslice = gbuf[:, 8:8 + nOut]
    masked = torch.where(act > 0, gslice, gslice * SLOPE).contiguous()
    assert masked.dtype == dtype
    f1, f2 = fn2_capi.correlation_backward_fused(ad, bd, buf, gbuf, 8, SLOPE, *params)
    u1, u2 = _bwd(ad, bd, masked, params, fn2_capi.FN2_CORR_AUTO, what)
    _same(f1, u1, what + " backward_fused grad_input1 vs the composition")
    _same(f2, u2, what + " backward_fused grad_input2 vs the composition")
    r1, r2 = L.corr_bwd64(ad, bd, masked, *params)
    ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), masked.abs(), *params)
    _check(f1, r1, _bwd_delta(dtype, r1, ab1, params), what + " grad_input1", ("backward fused", NAME[dtype], "general"))
    _check(f2, r2, _bwd_delta(dtype, r2, ab2, params), what + " grad_input2", ("backward fused", NAME[dtype], "general"))
    # slope 1 on a contiguous gradient: the plain backward
    gc = _gout("normal", (B, nOut, oH, oW), dtype, seed=sum(shape) + 2).to(dev)
    plain = torch.empty_like(gc)
    fn2_capi.correlation_forward(ad, bd, *params, out=plain)
    i1, i2 = fn2_capi.correlation_backward_fused(ad, bd, plain, gc, 0, 1.0, *params)
    p1, p2 = _bwd(ad, bd, gc, params, fn2_capi.FN2_CORR_AUTO, what)
    _same(i1, p1, what + " slope 1 grad_input1")
    _same(i2, p2, what + " slope 1 grad_input2")


# ------------------------------------------------------------------ e. the backward's second loop trip
def test_general_backward_second_grid_stride_trip(dev):
    """65 x 256 x 256 = 4,259,840 gradient elements against the 16384 x 256 = 4,194,304 lanes bwd_direct_launch's grid holds: the
    elements from flat index 4,194,304 on are computed by the second trip of corr_bwd_direct's loop."""
    import fn2_capi
    params, shape = (1, 1, 1, 1, 1), (1, 65, 256, 256)
    lanes = G.GRID_CAP_BLOCKS * G.BLOCK
    total = int(np.prod(shape))
    assert (lanes, total) == (4194304, 4259840) and lanes < total < 2 * lanes
    a, b = R.family_inputs(1, shape, seed=65)
    ad, bd = a.to(dev), b.to(dev)
    gd = R.grad_output("normal", _oshape(shape, params), seed=66).to(dev)
    g1, g2 = _bwd(ad, bd, gd, params, fn2_capi.FN2_CORR_DIRECT, "second trip")
    r1, r2 = L.corr_bwd64(ad, bd, gd, *params)
    ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), gd.abs(), *params)
    for g, r, ab, name in ((g1, r1, ab1, "grad_input1"), (g2, r2, ab2, "grad_input2")):
        tail = g.flatten()[lanes:]
        assert not bool(torch.isnan(tail).any()) and bool((tail != 0).any()), f"{name}: the second trip's elements"
        _check(g, r, _bwd_delta(F32, r, ab, params), f"second trip {name}", ("backward", "f32", "general, second trip"))


# ------------------------------------------------------------------ f. the Module
@pytest.mark.parametrize("case", [G.GRID[2], G.GRID[5]], ids=G.case_id)
def test_module_has_the_c_abi_bits(dev, case):
    import fn2_capi
    from networks.correlation_package.correlation import Correlation
    params, shape = case
    assert params in ((2, 1, 4, 1, 1), (4, 3, 5, 1, 2))
    a, b = R.family_inputs(1, shape, seed=sum(shape))
    ad, bd = a.to(dev), b.to(dev)
    want = _fwd(ad, bd, params, fn2_capi.FN2_CORR_AUTO, "C ABI forward")
    gd = R.grad_output("normal", tuple(want.shape), seed=2).to(dev)
    w1, w2 = _bwd(ad, bd, gd, params, fn2_capi.FN2_CORR_AUTO, "C ABI backward")
    ar, br = ad.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    out = Correlation(*params)(ar, br)
    _same(out.detach(), want, f"Correlation{params} forward")
    out.backward(gd)
    _same(ar.grad, w1, f"Correlation{params} grad_input1")
    _same(br.grad, w2, f"Correlation{params} grad_input2")


def test_module_with_stride1_2_runs_forward_and_rejects_backward(dev):
    import fn2_capi
    from networks.correlation_package.correlation import Correlation
    params, shape = G.GRID[8]
    assert params == (3, 3, 4, 2, 2)
    a, b = R.family_inputs(1, shape, seed=sum(shape))
    ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = Correlation(*params)(ad, bd)
    _same(out.detach(), _fwd(ad.detach(), bd.detach(), params, fn2_capi.FN2_CORR_AUTO, "C ABI forward"), f"Correlation{params} forward")
    with pytest.raises(RuntimeError, match=r"correlation_cuda\.backward: HIP call failed: flownet2_hip: parameter combination the reference "
                                           r"leaves undefined \(code -4\)"):
        out.backward(torch.ones_like(out))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ g. the fp32 matrix kernels at every radius
MFMA_FAMILIES = (1, 2, 3, 5, 7)
MFMA_FWD = [(md, s) for s in ((2, 64, 12, 16), (1, 32, 10, 18), (1, 64, 6, 72)) for md in (4, 8, 12, 16, 20)] + \
           [(6, (2, 64, 12, 16)), (14, (2, 64, 12, 16))]
MFMA_BWD = [(md, s) for s in ((2, 64, 12, 16), (1, 128, 10, 18), (8, 64, 64, 8)) for md in (4, 8, 12, 16, 20)]


def _mfma_id(c):
    return f"md{c[0]}-" + "x".join(map(str, c[1]))


@pytest.mark.parametrize("case", MFMA_FWD, ids=_mfma_id)
def test_matrix_forward_at_every_radius(dev, case):
    import fn2_capi
    md, shape = case
    B, C, H, W = shape
    params = (md, 1, md, 1, 2)
    NV, x3_ok, x4, tiles = G.mfma_nv(md), G.bf16x3_fwd_accepts(C, W, md), G.mfma_fwd_x4(W, md), G.mfma_x_tiles(W)
    # corr_forward_mfma_f32's own conditions, spelled out: which kernel each selector reaches on this case
    assert x3_ok == (C % 32 == 0 and W % 4 == 0 and W <= 64 and (md // 2) % 2 == 0)
    assert NV == {4: 2, 6: 3, 8: 3, 12: 4, 14: 5, 16: 5, 20: 6}[md]
    f32_kernel = "corr_fwd_mfma_dma<6>" if NV == 6 and x4 else f"corr_fwd_mfma_f32<NV = {NV}, x4 = {str(x4).lower()}>"
    print(f"  {_mfma_id(case)}: FN2_CORR_MFMA_F32 reaches {f32_kernel} on {tiles} x tile(s); FN2_CORR_MFMA_BF16X3 " +
          (f"reaches corr_fwd_mfma_bf16x3<NV = {NV}>" if x3_ok else "declines"))
    for fam in MFMA_FAMILIES:
        what = f"matrix fwd {_mfma_id(case)} family {fam}"
        a, b = R.family_inputs(fam, shape, seed=sum(shape) + md)
        ad, bd = a.to(dev), b.to(dev)
        assert ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
        ref = L.corr_fwd64(ad, bd, *params)
        absr = L.corr_fwd64(ad.abs(), bd.abs(), *params)
        f32 = _fwd(ad, bd, params, fn2_capi.FN2_CORR_MFMA_F32, what)
        _check(f32, ref, R.delta_fma_chain(ref, absr, C), what + " fp32 MFMA", ("forward", "f32", f"fp32 MFMA NV {NV}"))
        if x3_ok:
            x3 = _fwd(ad, bd, params, fn2_capi.FN2_CORR_MFMA_BF16X3, what)
            _check(x3, ref, R.delta_bf16x3(ref, absr, C), what + " bf16x3", ("forward", "f32", f"bf16x3 NV {NV}"))
        else:
            _fwd_declines(ad, bd, params, fn2_capi.FN2_CORR_MFMA_BF16X3, what + " bf16x3")
        if md < 20:   # (at md 20 AUTO's first choice is the f16x2 kernel: tests/test_gpu_f32_contract.py)
            _same(_fwd(ad, bd, params, fn2_capi.FN2_CORR_AUTO, what + " AUTO"), x3 if x3_ok else f32,
                  what + (" AUTO vs bf16x3" if x3_ok else " AUTO vs fp32 MFMA"))


@pytest.mark.parametrize("case", MFMA_BWD, ids=_mfma_id)
def test_matrix_backward_at_every_radius(dev, case):
    """FN2_CORR_MFMA_F32 and the debug tunes 101 (32-channel groups forced) and 102 (64-channel groups forced): each inside the
    fma chain's bracket; FN2_CORR_MFMA_F32 has the bits of the group size that the restated occupancy test predicts."""
    import fn2_capi
    md, shape = case
    B, C, H, W = shape
    params = (md, 1, md, 1, 2)
    NV, n = G.mfma_nv(md), L.n_bwd(md, 2, 1)
    assert C % 64 == 0 and G.bwd_groups64(B, C, H, W, tune=2) and not G.bwd_groups64(B, C, H, W, tune=1)
    keeps64 = G.bwd_groups64(B, C, H, W)
    assert keeps64 == (shape == (8, 64, 64, 8))
    print(f"  {_mfma_id(case)}: FN2_CORR_MFMA_F32 reaches mb::launch_nv<{4 if keeps64 else 2}> ({64 if keeps64 else 32}-channel groups), "
          f"101 launch_nv<2>, 102 launch_nv<4>, NV = {NV}")
    for fam in MFMA_FAMILIES:
        what = f"matrix bwd {_mfma_id(case)} family {fam}"
        a, b = R.family_inputs(fam, shape, seed=sum(shape) + md)
        ad, bd = a.to(dev), b.to(dev)
        gd = R.grad_output("normal", _oshape(shape, params), seed=sum(shape) + fam).to(dev)
        r1, r2 = L.corr_bwd64(ad, bd, gd, *params)
        ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), gd.abs(), *params)
        got = {}
        for algo, name in ((fn2_capi.FN2_CORR_MFMA_F32, "fp32 MFMA"), (101, "32-channel groups"), (102, "64-channel groups")):
            g1, g2 = got[algo] = _bwd(ad, bd, gd, params, algo, f"{what} {name}")
            key = ("backward", "f32", f"{name} NV {NV}")
            _check(g1, r1, R.delta_fma_chain(r1, ab1, n, C), f"{what} {name} grad_input1", key)
            _check(g2, r2, R.delta_fma_chain(r2, ab2, n, C), f"{what} {name} grad_input2", key)
        for g, w in zip(got[fn2_capi.FN2_CORR_MFMA_F32], got[102 if keeps64 else 101]):
            _same(g, w, f"{what}: FN2_CORR_MFMA_F32 vs the predicted group size")


# ------------------------------------------------------------------ the report
def test_report_worst_ratios():
    """The largest err / delta of this run per (quantity, dtype, kernel): measured, recorded in DESIGN.md 4.4, not asserted (the
    brackets above are the assertions)."""
    for (quantity, dtype, kernel), ratio in sorted(WORST.items()):
        print(f"  worst err/delta: {quantity:15s} {dtype:5s} {kernel:32s} {ratio:.3g}")
