"""The float32 warp and norm kernels (csrc/resample2d.hip, csrc/channelnorm.hip) pinned per element: every output against the float64
reference and bound of tests/warp_contract_ref.py (derivations there; tests/test_warp_contract_host.py holds the oracle to the same
brackets), forward / grad_flow / ChannelNorm bit for bit against the oracle, the tiled kernels bit for bit against the untiled ones
(the debug library's entry points with flag 0x100 only), the fused rows bit for bit against the unfused HIP layers.  Outputs start as
NaN inside a sentinel-guarded allocation that must be untouched afterwards.  Every test prints its worst err / delta; the last one
reports the largest per quantity and kernel branch.

Bit-identity to the oracle, as first run on an MI355X (both sides are built with -ffp-contract=off):
  * grad_flow, the nearest forward, ChannelNorm forward and backward (float32 and float64): bit-identical, asserted.
  * the bilinear forward: NOT bit-identical -- 324 583 of 6 734 756 elements of these cases differ, by up to 131 072 ulp where the four
    terms cancel (16 384 ulp on the shapes the host test runs).  The operation: the BR term.  The reference writes `(alpha) * (beta) * I`
    (resample2d_kernel.cu:59) without a double literal, so alpha * beta and its product with I are fp32 operations, two roundings;
    the kernels form all four weights in double (bilinear_weights) and round the term once.  The bracket stays the assertion (worst
    err / delta 0.84); on top of it the kernels' own sequence, restated operation by operation in numpy, is asserted bit for bit, and
    the oracle's bits wherever the BR terms vanish and at every wild pixel (those do hold).
  * ChannelNorm forward was not bit-identical when this file was written: 7 of 768 norms of (2, 3, 16, 24) and 7 of 180 of (3, 5, 6, 10)
    were one ulp off, graded input, first at element (0, 0, 9, 14).  `__fsqrt_rn` is HIP's native square root and the vector kernel got
    the bare v_sqrt_f32; the kernels now call sqrtf (correctly rounded) and the assertion holds."""
import ctypes

import numpy as np
import pytest
import torch

import warp_contract_ref as R
from resample_det_ref import warped_grad

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 64
UNTILED = 0x100
WORST = {}
# The bilinear forward against the oracle: [elements that differ, elements compared, worst distance in ulp] over this module's cases.
# The reference forms the BR term `(alpha) * (beta) * I` (resample2d_kernel.cu:59) in fp32 -- no double literal in it: alpha * beta is
# rounded, then the product with I -- and the oracle restates that; the kernels form all four weights in double (bilinear_weights) and
# round each term once.  So the bits differ where that one term rounds differently: the bracket is the assertion, together with the
# kernels' sequence in numpy (bit for bit) and the oracle's bits wherever the BR terms vanish.
BILINEAR_VS_ORACLE = [0, 0, 0]


def _note(quantity, where, ratio):
    WORST[(quantity, where)] = max(WORST.get((quantity, where), 0.0), ratio)


def _guarded(shape, dev, fill=None, off=0, dtype=torch.float32):
    """a `shape` view `off` elements past a 256-byte boundary inside a sentinel-filled allocation, holding NaN or `fill`"""
    n = int(np.prod(shape))
    whole = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=dtype, device=dev)
    view = whole[GUARD + off:GUARD + off + n].view(shape)
    if fill is None:
        view.fill_(float("nan"))
    else:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill)).to(dtype).view(shape))
    return view, whole


def _untouched(whole, view, what):
    n, lo = view.numel(), view.storage_offset()
    assert bool((whole[:lo] == SENTINEL).all()) and bool((whole[lo + n:] == SENTINEL).all()), f"{what}: wrote outside its output"


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _strides(t):
    return (ctypes.c_int64 * 4)(*t.stride())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _forward(img, flow, out, ks, bilinear, untiled=False):
    import fn2_capi
    B, C, Hi, Wi = img.shape
    H, W = flow.shape[2:]
    if untiled:
        rc = fn2_capi.debug_lib().fn2_debug_resample2d_forward(_p(img), _strides(img), _p(flow), _p(out), B, C, Hi, Wi, H, W, ks,
                                                                int(bilinear), UNTILED, _stream(img))
    else:
        rc = fn2_capi.lib().fn2_resample2d_forward(_p(img), _strides(img), _p(flow), _p(out), B, C, Hi, Wi, H, W, ks, int(bilinear), _stream(img))
    fn2_capi.check(rc, "resample2d forward")
    torch.cuda.synchronize()


def _backward(img, flow, gout, gimg, gflow, ks, untiled=False):
    import fn2_capi
    B, C, Hi, Wi = img.shape
    H, W = flow.shape[2:]
    if untiled:
        rc = fn2_capi.debug_lib().fn2_debug_resample2d_backward(_p(img), _strides(img), _p(flow), _p(gout), _p(gimg), _p(gflow), B, C, Hi, Wi,
                                                                 H, W, ks, 1, UNTILED, _stream(img))
    else:
        rc = fn2_capi.lib().fn2_resample2d_backward(_p(img), _strides(img), _p(flow), _p(gout), _p(gimg), _p(gflow), B, C, Hi, Wi, H, W, ks, 1,
                                                    _stream(img))
    fn2_capi.check(rc, "resample2d backward")
    torch.cuda.synchronize()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _image(case, dev, variant):
    """the case's image on the device: dense and aligned, 4 bytes past a 16-byte boundary, or a channel slice x[:, 3:]"""
    B, C, Hi, Wi = case.img_shape
    if variant == "img+4":
        view, _ = _guarded(case.img_shape, dev, case.img, off=1)
        assert view.data_ptr() % 16 == 4
        return view
    if variant == "slice":
        x = torch.full((B, C + 3, Hi, Wi), 1.0e30, device=dev)
        x[:, 3:] = _dev(case.img, dev)
        return x[:, 3:]
    return _dev(case.img, dev)


def _oracle_fwd(oracle, case, bilinear):
    return case.cached(("oracle fwd", bilinear), lambda: oracle.resample_fwd(case.img, case.flow, case.ks, bilinear))


def _oracle_bwd(oracle, case):
    return case.cached("oracle bwd", lambda: oracle.resample_bwd(case.img, case.flow, case.gout, case.ks, True))


def _bits(got, want, what):
    eq = R.same_bits(got, want)
    assert eq.all(), (f"{what}: {int((~eq).sum())} of {eq.size} elements differ in their bits, worst distance {R.ulp_distance(got, want)} ulp; "
                      f"first at {np.unravel_index(int(np.flatnonzero(~eq.ravel())[0]), eq.shape)}")


def _check_case(case, dev, oracle, variant=None, vs_untiled=None):
    """assertions 1-4 for one case; `variant`: how the image, the flow and the outputs are laid out"""
    B, C, Hi, Wi = case.img_shape
    H, W = case.H, case.W
    where = R.branch(case) if variant is None else f"layout '{variant}'"
    off = 1 if variant == "flow+1" else 0
    img = _image(case, dev, variant)
    flow, _ = _guarded((B, 2, H, W), dev, case.flow, off=off)
    vs_untiled = case.tiled if vs_untiled is None else vs_untiled
    line = [case.id + (f" [{variant}]" if variant else "")]
    for bilinear in (True, False):
        mode = "bilinear" if bilinear else "nearest"
        out, whole = _guarded((B, C, H, W), dev, off=off)
        _forward(img, flow, out, case.ks, bilinear)
        _untouched(whole, out, f"{case.id} forward {mode}")
        got = out.cpu().numpy()
        ref, delta, wild = case.fwd64(bilinear)
        r = R.ratio_and_check(got, ref, delta, ~wild[:, None], f"{case.id} forward {mode}")
        orc = _oracle_fwd(oracle, case, bilinear)
        if bilinear:
            # not bit-identical to the oracle: see BILINEAR_VS_ORACLE.  The kernels' own operation sequence, restated in numpy, pins
            # the bits instead; the oracle's bits are required wherever the BR terms vanish.
            seq, br_zero = case.seq32
            _bits(got, seq, f"{case.id} forward bilinear against the kernels' operation sequence in numpy")
            eq = R.same_bits(got, orc)
            assert eq[br_zero].all(), f"{case.id} forward bilinear differs from the oracle where the BR term is zero"
            # wild pixels have no bracket: the oracle's bits, NaN as a mask (a NaN BR term makes the whole sum NaN on both sides)
            at_wild = np.broadcast_to(wild[:, None], eq.shape)
            assert eq[at_wild].all(), f"{case.id} forward bilinear differs from the oracle at {int((~eq[at_wild]).sum())} wild pixels"
            BILINEAR_VS_ORACLE[0] += int((~eq).sum())
            BILINEAR_VS_ORACLE[1] += eq.size
            BILINEAR_VS_ORACLE[2] = max(BILINEAR_VS_ORACLE[2], R.ulp_distance(got, orc))
        else:
            _bits(got, orc, f"{case.id} forward nearest against the oracle")
        if vs_untiled:
            out2, whole2 = _guarded((B, C, H, W), dev, off=off)
            _forward(img, flow, out2, case.ks, bilinear, untiled=True)
            _untouched(whole2, out2, f"{case.id} untiled forward {mode}")
            _bits(got, out2.cpu().numpy(), f"{case.id} forward {mode}, tiled against untiled")
        _note(f"forward {mode}", where, r)
        line.append(f"forward {mode} {r:.3f}")
    if case.backward:
        gout = _dev(case.gout, dev)
        oimg, oflow = _oracle_bwd(oracle, case)
        for with_prefill in (False, True):
            b = case.bwd64(with_prefill)
            pre = case.prefill if with_prefill else np.zeros(case.img_shape, np.float32)
            gimg, wi = _guarded(case.img_shape, dev, pre)
            gflow, wf = _guarded((B, 2, H, W), dev, off=off)
            _backward(img, flow, gout, gimg, gflow, case.ks)
            _untouched(wi, gimg, f"{case.id} grad_input1")
            _untouched(wf, gflow, f"{case.id} grad_flow")
            gi, gf = gimg.cpu().numpy(), gflow.cpu().numpy()
            r1 = R.ratio_and_check(gi, b.gimg, b.gimg_delta, ~b.excluded[:, None], f"{case.id} grad_input1 (prefill {with_prefill})")
            keep = ~b.reached & ~b.excluded[:, None]
            assert R.same_bits(gi, pre)[keep].all(), f"{case.id}: a cell no pixel reaches lost its prefill"
            r2 = R.ratio_and_check(gf, b.gflow, b.gflow_delta, ~b.wild[:, None], f"{case.id} grad_flow")
            _bits(gf, oflow, f"{case.id} grad_flow against the oracle")
            if vs_untiled:
                gimg2, wi2 = _guarded(case.img_shape, dev, pre)
                gflow2, wf2 = _guarded((B, 2, H, W), dev, off=off)
                _backward(img, flow, gout, gimg2, gflow2, case.ks, untiled=True)
                _untouched(wi2, gimg2, f"{case.id} untiled grad_input1")
                _untouched(wf2, gflow2, f"{case.id} untiled grad_flow")
                _bits(gf, gflow2.cpu().numpy(), f"{case.id} grad_flow, tiled against untiled")
                r3 = R.ratio_and_check(gimg2.cpu().numpy(), b.gimg, b.gimg_delta, ~b.excluded[:, None], f"{case.id} untiled grad_input1")
                _note("grad_input1", "untiled kernel on a tileable shape (resample_bwd_kernel)", r3)
            _note("grad_input1", where, r1)
            _note("grad_flow", where, r2)
            line.append(f"grad_input1{' prefilled' if with_prefill else ''} {r1:.3f} grad_flow {r2:.3f}")
    print("err / delta:", ", ".join(line))


# ------------------------------------------------------------------ Resample2d
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_resample2d_contract(dev, oracle, case):
    """Assertions 1-4 of the contract on every family x shape: forward (bilinear, nearest) and grad_flow bit-identical to the oracle
    and inside their float64 brackets, grad_input1 per cell inside its bracket with zero and with a graded prefill, unreached cells
    keeping the prefill, and on tileable shapes the tiled kernels bit-identical to the untiled ones -- wherever the `follow` and
    `window` families sent the windows."""
    assert case.excluded_share() <= R.EXCLUDED_CAP
    if case.img_shape == R.BIG_SHAPE:
        assert R.tile_height(1, case.H, (case.W + 63) // 64) == 48 and R.branch(case).startswith("tiled, 48 rows")
    _check_case(case, dev, oracle)


FALLBACKS = [(shape, fam, variant) for shape in ((2, 2, 16, 32), (2, 3, 33, 68)) for fam in ("noise", "grid")
             for variant in ("img+4", "slice", "flow+1")] + [((2, 3, 8, 36), fam, "flow+1") for fam in ("noise", "grid")]


@pytest.mark.parametrize("shape,family,variant", FALLBACKS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_resample2d_layouts(dev, oracle, shape, family, variant):
    """The same results from every layout of a tileable shape: the image 4 bytes past a 16-byte boundary (untiled kernels), the image
    as a channel slice x[:, 3:] (tiled kernels with a batch stride of their own; the three leading channels hold 1e30), flow and
    outputs one element off a 16-byte boundary (no 16-byte accesses to them; resample_fwd_kernel<1> on an untiled shape)."""
    case = next(c for c in R.CASES if c.img_shape == shape and c.family == family and c.ks == 1 and c.seed == 0)
    _check_case(case, dev, oracle, variant, vs_untiled=False)


# ------------------------------------------------------------------ ChannelNorm
def _chnorm(x, go_view, dtype_code):
    import fn2_capi
    B, C, H, W = x.shape
    out, wo = _guarded((B, 1, H, W), x.device, dtype=x.dtype)
    fn2_capi.check(fn2_capi.lib().fn2_channelnorm_forward(_p(x), _p(out), dtype_code, B, C, H, W, _stream(x)), "channelnorm forward")
    gin, wg = _guarded(x.shape, x.device, dtype=x.dtype)
    fn2_capi.check(fn2_capi.lib().fn2_channelnorm_backward(_p(x), _p(out), _p(go_view), _strides(go_view), _p(gin), dtype_code, B, C, H, W,
                                                           _stream(x)), "channelnorm backward")
    torch.cuda.synchronize()
    _untouched(wo, out, "channelnorm forward")
    _untouched(wg, gin, "channelnorm backward")
    return out.cpu().numpy(), gin.cpu().numpy()


@pytest.mark.parametrize("shape", R.CHNORM_SHAPES)
@pytest.mark.parametrize("go_layout", ["dense", "channel_slice", "transposed"])
def test_channelnorm_contract(dev, oracle, shape, go_layout):
    """Assertion 5: float32 ChannelNorm forward and backward on graded inputs inside their brackets and bit-identical to the oracle,
    the exactly-zero pixel gives 0 (not NaN) both ways, float64 bit-identical to the oracle; vector kernels (H W % 4 == 0), scalar
    kernels ((1, 2, 7, 9), and a grad_output with a pixel stride), a grad_output with a batch stride of its own."""
    import fn2_capi
    B, C, H, W = shape
    x = R.chnorm_input(shape)
    go = np.ascontiguousarray(R.graded((B, 2, H, W), 0)[:, 1:])

    def layout(g):
        if go_layout == "channel_slice":
            full = torch.full((B, 2, H, W), 1.0e30, dtype=g.dtype, device=dev)
            full[:, 1:2] = g
            return full[:, 1:2]
        if go_layout == "transposed":
            return g.transpose(2, 3).contiguous().transpose(2, 3)
        return g
    out, gin = _chnorm(_dev(x, dev), layout(_dev(go, dev)), fn2_capi.FN2_F32)
    ref, delta = R.chnorm_fwd64(x)
    r1 = R.ratio_and_check(out, ref, delta, None, f"{shape} chnorm forward")
    o_out = oracle.chnorm_fwd(x)
    _bits(out, o_out, f"{shape} chnorm forward against the oracle")
    ref, delta = R.chnorm_bwd64(x, out, go)
    r2 = R.ratio_and_check(gin, ref, delta, None, f"{shape} chnorm backward")
    _bits(gin, oracle.chnorm_bwd(x, o_out, go), f"{shape} chnorm backward against the oracle")
    assert out[0, 0, 0, 0] == 0 and not gin[0, :, 0, 0].any() and not np.isnan(gin).any()
    where = "vector kernels" if (H * W) % 4 == 0 and go_layout != "transposed" else "scalar kernels"
    _note("chnorm forward", "vector kernel" if (H * W) % 4 == 0 else "scalar kernel", r1)
    _note("chnorm backward", where, r2)
    print(f"err / delta: {shape} {go_layout}: chnorm forward {r1:.3f}, backward {r2:.3f}")
    # float64: bit-identical to the oracle
    x64 = x.astype(np.float64) * (1 + 2.0 ** -30) + R.graded(shape, 5).astype(np.float64) * 2.0 ** -40
    x64[0, :, 0, 0] = 0
    go64 = go.astype(np.float64) * (1 + 2.0 ** -31)
    out64, gin64 = _chnorm(_dev(x64, dev), layout(_dev(go64, dev)), fn2_capi.FN2_F64)
    o64 = oracle.chnorm_fwd(x64)
    assert np.array_equal(out64.view(np.uint64), o64.view(np.uint64))
    assert np.array_equal(gin64.view(np.uint64), oracle.chnorm_bwd(x64, o64, go64).view(np.uint64))
    assert out64[0, 0, 0, 0] == 0 and not gin64[0, :, 0, 0].any()


# ------------------------------------------------------------------ fused rows
@pytest.mark.parametrize("case", R.FUSED_CASES, ids=lambda c: "pair-" + c.id)
@pytest.mark.parametrize("bilinear", [True, False])
def test_fused_rows_contract(dev, case, bilinear):
    """Assertion 6: warp_diff_norm_cat, warp_diff_norm and their backwards on the grid, window, follow and wild families bit-identical
    to the unfused HIP layers (NaN where they have NaN), and the second image's gradient inside the grad_input1 bound -- its prefill
    is the concat gradient's slice, its grad_out the warped image's gradient as the fused kernel forms it."""
    import fn2_capi
    from networks.channelnorm_package.channelnorm import ChannelNorm
    from networks.resample2d_package.resample2d import Resample2d
    assert case.excluded_share() <= R.EXCLUDED_CAP
    B, C, H, W = case.img_shape
    pair = R.graded((B, 2 * C, H, W), case.seed + 10)
    gcat = R.graded((B, 3 * C + 3, H, W), case.seed + 11)
    gn = R.graded((B, 1, H, W), case.seed + 12)
    xd, fd, gd, gnd = _dev(pair, dev), _dev(case.flow, dev), _dev(gcat, dev), _dev(gn, dev)
    # the unfused layers under autograd, in the reference model's statement order
    x, f = xd.clone().requires_grad_(True), fd.clone().requires_grad_(True)
    res = Resample2d(1, bilinear)(x[:, C:], f)
    unf = torch.cat((x, res, f / 20.0, ChannelNorm()(x[:, :C] - res)), dim=1)
    unf.backward(gd)
    # the entry points fn2_capi.warp_diff_norm_cat / _backward / warp_diff_norm / _backward wrap, called as those wrappers call them
    # but with NaN-prefilled outputs inside sentinel-guarded allocations (the wrappers allocate their outputs themselves)
    lib, bil, div, st = fn2_capi.lib(), int(bilinear), ctypes.c_float(20.0), _stream(xd)
    got, w0 = _guarded((B, 3 * C + 3, H, W), dev)
    fn2_capi.check(lib.fn2_warp_diff_norm_cat(_p(xd), _p(fd), _p(got), div, B, C, H, W, bil, st), "fn2_warp_diff_norm_cat")
    torch.cuda.synchronize()
    _untouched(w0, got, f"{case.id} warp_diff_norm_cat")
    _bits(got.cpu().numpy(), unf.detach().cpu().numpy(), f"{case.id} warp_diff_norm_cat")
    gp, w1 = _guarded((B, 2 * C, H, W), dev)
    gf, w2 = _guarded((B, 2, H, W), dev)
    fn2_capi.check(lib.fn2_warp_diff_norm_cat_backward(_p(xd), _p(fd), _p(got), _p(gd), _p(gp), _p(gf), div, B, C, H, W, bil, st),
                   "fn2_warp_diff_norm_cat_backward")
    torch.cuda.synchronize()
    _untouched(w1, gp, f"{case.id} warp_diff_norm_cat_backward grad_pair")
    _untouched(w2, gf, f"{case.id} warp_diff_norm_cat_backward grad_flow")
    _bits(gf.cpu().numpy(), f.grad.cpu().numpy(), f"{case.id} warp_diff_norm_cat_backward grad_flow")
    _bits(gp[:, :C].cpu().numpy(), x.grad[:, :C].cpu().numpy(), f"{case.id} warp_diff_norm_cat_backward first image")
    gw = warped_grad(pair, got.cpu().numpy(), gcat)
    b = R.resample_bwd64(pair[:, C:], case.flow, gw, 1, prefill=gcat[:, C:2 * C])
    r = R.ratio_and_check(gp[:, C:].cpu().numpy(), b.gimg, b.gimg_delta, ~b.excluded[:, None], f"{case.id} fused grad of the second image")
    r0 = R.ratio_and_check(x.grad[:, C:].cpu().numpy(), b.gimg, b.gimg_delta, ~b.excluded[:, None], f"{case.id} unfused grad of the second image")
    _note("grad_input1", "fused row " + ("(resample_bwd_c3x, fused)" if C == 3 and R.tileable(H, W, H, W) else "(warp_diff_norm_cat_bwd_kernel)"), r)
    # the norm-only row
    x2, f2 = xd, fd.clone().requires_grad_(True)
    n_unf = ChannelNorm()(x2[:, :C] - Resample2d(1, bilinear)(x2[:, C:], f2))
    n_unf.backward(gnd)
    n2, w3 = _guarded((B, 1, H, W), dev)
    fn2_capi.check(lib.fn2_warp_diff_norm(_p(xd), _p(fd), _p(n2), B, C, H, W, bil, st), "fn2_warp_diff_norm")
    torch.cuda.synchronize()
    _untouched(w3, n2, f"{case.id} warp_diff_norm")
    _bits(n2.cpu().numpy(), n_unf.detach().cpu().numpy(), f"{case.id} warp_diff_norm")
    gf2, w4 = _guarded((B, 2, H, W), dev)
    fn2_capi.check(lib.fn2_warp_diff_norm_backward(_p(xd), _p(fd), _p(n2), _p(gnd), _p(gf2), B, C, H, W, bil, st), "fn2_warp_diff_norm_backward")
    torch.cuda.synchronize()
    _untouched(w4, gf2, f"{case.id} warp_diff_norm_backward")
    _bits(gf2.cpu().numpy(), f2.grad.cpu().numpy(), f"{case.id} warp_diff_norm_backward")
    print(f"err / delta: pair {case.id} bilinear={bilinear}: second image's gradient fused {r:.3f}, unfused {r0:.3f}")


def test_report_worst_ratios(dev, oracle):
    """the largest err / delta per quantity and kernel branch over this module's tests (each <= 1 by the assertions above); run alone, or
    in a worker that ran none of them, it runs one small tiled case itself so that it never passes on nothing"""
    if not WORST:
        _check_case(next(c for c in R.CASES if c.tiled and c.family == "grid"), dev, oracle)
    assert WORST and BILINEAR_VS_ORACLE[1] > 0
    for (quantity, where), v in sorted(WORST.items()):
        print(f"worst err / delta: {quantity:18s} {where}: {v:.3f}")
    d = BILINEAR_VS_ORACLE
    print(f"forward bilinear against the oracle: {d[0]} of {d[1]} elements differ in their bits, at most {d[2]} ulp")
    assert all(v <= 1.0 for v in WORST.values())
