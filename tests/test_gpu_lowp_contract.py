"""The half and bfloat16 kernels against their rounding contract, element by element (include/flownet2_hip.h at FN2_BF16 and
FN2_CORR_MFMA_F16X2): exact products, fp32 sums, one rounding to the tensor's type.  Every output element must lie in the
bracket of tests/lowp_ref.py -- the float64 result, widened by the fp32 summation bound of that element (it scales with the
element's own sum of |terms|, not with the largest output), rounded once -- so a kernel that rounds a product, a partial sum or
1/C to 16 bits fails here (tests/test_lowp_ref_host.py shows the older global bounds accepting such a kernel).

Every case also checks that no output was left unwritten (outputs prefilled with NaN) and which kernel ran, by a bit-identical
pair of results; with the preconditions in csrc/corr_params.h that names the kernel:
  narrow / column-window (correlation_f16_fwd.hip) and the narrow backward (correlation_f16_bwd.hip): AUTO == FN2_CORR_MFMA_F16X2;
  general (correlation_direct.hip): AUTO == FN2_CORR_DIRECT, and FN2_CORR_MFMA_F16X2 returns FN2_EUNSUPPORTED;
  widened (W > 64 backward in the binding): the fp32 f16x2 kernel on the widened operands, narrowed once."""
import pytest
import torch

import lowp_ref as L

pytestmark = pytest.mark.gpu

HF, BF = torch.float16, torch.bfloat16
DTYPES = [HF, BF]
CORR = L.CORR
FAMILIES = (1, 2, 3, 4, 5)
SLOPE = 0.1
EUNSUPPORTED = "code -4"

# forward: narrow kernel (W <= 64) and column-window kernel (W > 64); C in {128, 256, 384, 512}: 384 runs the division by C
FWD_NARROW = [(1, 128, 2, 8), (1, 384, 2, 56), (2, 128, 46, 56), (1, 512, 48, 64), (2, 256, 56, 64)]
FWD_WIDE = [(1, 384, 48, 72), (2, 128, 46, 128), (1, 256, 2, 136), (1, 512, 56, 200), (8, 256, 56, 128)]   # last: Sintel conv3
# backward: narrow matrix kernel (W <= 64); wider maps: the widened fp32 path.  C in {64, 192, 256, 320}: 192 and 320 divide
BWD_NARROW = [(1, 64, 2, 8), (2, 192, 46, 56), (1, 320, 48, 64), (4, 256, 56, 64)]
BWD_WIDE = [(1, 192, 48, 72), (2, 64, 46, 128), (1, 320, 2, 136)]
# the general kernel: C the matrix kernels decline, and kernel_size 3 / stride1 2
GEN_FWD = [(CORR, (2, 96, 16, 24), FAMILIES), ((3, 3, 4, 2, 2), (2, 32, 16, 20), (1, 2)), ((3, 3, 4, 1, 2), (2, 32, 16, 20), (1, 2))]
GEN_BWD = [(CORR, (1, 96, 8, 16), (1, 2)), ((3, 3, 4, 1, 2), (2, 32, 12, 14), (1, 2))]


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _structural_zeros(H, W, params, dev):
    """Outputs whose every term falls in the padding: zero in the float64 reference on a constant input."""
    one = torch.ones(1, 1, H, W, dtype=torch.float64, device=dev)
    return L.corr_fwd64(one, one, *params) == 0


def _fwd_ref(ad, bd, params, dtype, kernel):
    """float64 forward and its error bound for `kernel`."""
    C, k = ad.shape[1], params[1]
    ref = L.corr_fwd64(ad, bd, *params)
    absr = L.corr_fwd64(ad.abs(), bd.abs(), *params)
    return ref, (L.delta_fwd_direct_half if kernel == "general" and dtype == HF else L.delta_fwd)(ref, absr, C, k)


def _check_forward(dev, a, b, params, dtype, kernel, what):
    import fn2_capi
    ad, bd = a.to(dev), b.to(dev)
    B, C, H, W = a.shape
    nOut, oH, oW = L.out_shape(H, W, *params)
    out = _nan((B, nOut, oH, oW), dtype, dev)
    fn2_capi.correlation_forward(ad, bd, *params, out=out)                                   # AUTO
    assert not torch.isnan(out).any(), f"{what}: unwritten output elements"
    ref, delta = _fwd_ref(ad, bd, params, dtype, kernel)
    lo, hi = L.bracket(ref, delta, dtype)
    L.check_bracket(out, lo, hi, what)
    zeros = _structural_zeros(H, W, params, dev).expand_as(out)
    assert bool((out[zeros] == 0).all()), f"{what}: an all-padding output is not exactly zero"
    # which kernel ran
    if kernel == "matrix":
        sel = fn2_capi.correlation_forward(ad, bd, *params, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
        assert torch.equal(sel, out), what
    else:
        direct = fn2_capi.correlation_forward(ad, bd, *params, algo=fn2_capi.FN2_CORR_DIRECT)
        assert torch.equal(direct, out), what
        with pytest.raises(RuntimeError, match=EUNSUPPORTED):
            fn2_capi.correlation_forward(ad, bd, *params, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
    # fused LeakyReLU + store into a concat slice: the kernel's own rounding sequence, and nothing outside the slice touched
    g = torch.Generator(device=dev).manual_seed(B + C + H + W)
    buf = torch.randn((B, 8 + nOut + 3, oH, oW), generator=g, device=dev).to(dtype)
    buf[:, 8:8 + nOut] = float("nan")
    before = buf.clone()
    fn2_capi.correlation_forward_fused(ad, bd, buf, 8, SLOPE, *params)
    assert torch.equal(buf[:, :8].view(torch.int16), before[:, :8].view(torch.int16)), what
    assert torch.equal(buf[:, 8 + nOut:].view(torch.int16), before[:, 8 + nOut:].view(torch.int16)), what
    fused = buf[:, 8:8 + nOut]
    assert not torch.isnan(fused).any(), f"{what}: unwritten fused output elements"
    post = (L.leaky_matrix if kernel == "matrix" else L.leaky_general)(SLOPE, dtype)
    flo, fhi = L.bracket(ref, delta, dtype, post=post)
    L.check_bracket(fused, flo, fhi, what + " fused")
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("case", FWD_NARROW + FWD_WIDE)
def test_forward_matrix_kernels(dev, case, dtype):
    """Narrow (W <= 64) and column-window (W > 64) kernels, input families 1-5, plain and fused."""
    for fam in FAMILIES:
        a, b = L.family_inputs(fam, case, dtype, seed=sum(case))
        _check_forward(dev, a, b, CORR, dtype, "matrix", f"{case} family {fam}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("gen", GEN_FWD, ids=["C96", "k3s1_2", "k3s1_1"])
def test_forward_general_kernel(dev, gen, dtype):
    params, shape, fams = gen
    for fam in fams:
        a, b = L.family_inputs(fam, shape, dtype, seed=sum(shape))
        _check_forward(dev, a, b, params, dtype, "general", f"{params} {shape} family {fam}")


def test_forward_half_overflow(dev):
    """Half matrix kernel with products formed exactly in fp32: inputs of magnitude 180..300 put some outputs past 65520 (+-inf
    after the one rounding) and keep others below; the bracket predicts which, and exactly those are infinite."""
    import fn2_capi
    B, C, H, W = 1, 128, 6, 8
    g = torch.Generator().manual_seed(21)
    vals = torch.tensor([180.0, 200.0, 224.0, 240.0, 250.0, 256.0, 260.0, 300.0])
    v = vals[torch.randint(0, len(vals), (B, 1, H, W), generator=g)]
    s = torch.where(torch.rand(B, 1, H, W, generator=g) < 0.5, -1.0, 1.0)
    a = v.expand(B, C, H, W).contiguous().to(HF).to(dev)
    b = (s * v).expand(B, C, H, W).contiguous().to(HF).to(dev)
    out = _nan((B, 441, H, W), HF, dev)
    fn2_capi.correlation_forward(a, b, *CORR, out=out)
    lo, hi = L.bracket(*_fwd_ref(a, b, CORR, HF, "matrix"), HF)
    L.check_bracket(out, lo, hi, "half overflow")
    assert not bool((torch.isinf(lo) != torch.isinf(hi)).any()), "a reference within the bound of the overflow threshold"
    n_inf, n_fin = int(torch.isinf(out).sum()), int((torch.isfinite(out) & (out != 0)).sum())
    assert n_inf > 0 and n_fin > 0 and bool((out == -float("inf")).any()) and bool((out == float("inf")).any())
    assert torch.equal(torch.isinf(out), torch.isinf(lo))
    assert torch.equal(fn2_capi.correlation_forward(a, b, *CORR, algo=fn2_capi.FN2_CORR_MFMA_F16X2), out)


# ------------------------------------------------------------------ backward
def _bwd_ref(ad, bd, gd, params, kernel):
    r1, r2 = L.corr_bwd64(ad, bd, gd, *params)
    ab1, ab2 = L.corr_bwd64(ad.abs(), bd.abs(), gd.abs(), *params)
    if kernel == "widened":
        d1, d2 = L.delta_bwd_widened(ad, bd, gd, r1, r2, ab1, ab2)
    else:
        d1 = L.delta_bwd(r1, ab1, params[2], params[4], params[1])
        d2 = L.delta_bwd(r2, ab2, params[2], params[4], params[1])
    return (r1, d1), (r2, d2)


def _check_backward(dev, a, b, go, params, dtype, kernel, what):
    import correlation_cuda
    import fn2_capi
    ad, bd, gd = a.to(dev), b.to(dev), go.to(dev)
    g1, g2 = _nan(a.shape, dtype, dev), _nan(a.shape, dtype, dev)
    if kernel == "widened":
        correlation_cuda.backward(ad, bd, torch.empty(0, dtype=dtype, device=dev), torch.empty(0, dtype=dtype, device=dev), gd, g1, g2,
                                  *params, 1)
        w1, w2 = correlation_cuda.backward_alloc(ad, bd, gd, *params, 1)
        assert torch.equal(w1, g1) and torch.equal(w2, g2), what
        f1, f2 = fn2_capi.correlation_backward(ad.float(), bd.float(), gd.float(), *params, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
        assert torch.equal(f1.to(dtype), g1) and torch.equal(f2.to(dtype), g2), what           # the fp32 f16x2 kernel, narrowed
    else:
        fn2_capi.correlation_backward(ad, bd, gd, *params, out=(g1, g2))                        # AUTO
        if kernel == "matrix":
            s1, s2 = fn2_capi.correlation_backward(ad, bd, gd, *params, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
        else:
            s1, s2 = fn2_capi.correlation_backward(ad, bd, gd, *params, algo=fn2_capi.FN2_CORR_DIRECT)
            with pytest.raises(RuntimeError, match=EUNSUPPORTED):
                fn2_capi.correlation_backward(ad, bd, gd, *params, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
        assert torch.equal(s1, g1) and torch.equal(s2, g2), what
    for name, got, (ref, delta) in zip(("grad_input1", "grad_input2"), (g1, g2), _bwd_ref(ad, bd, gd, params, kernel)):
        assert not torch.isnan(got).any(), f"{what} {name}: unwritten elements"
        lo, hi = L.bracket(ref, delta, dtype)
        L.check_bracket(got, lo, hi, f"{what} {name}")


def _bwd_runs(shape, dtype, seed, fams=FAMILIES, grads=("leaky", "window")):
    """(in1, in2, gradOutput, label): every input family with a normal gradOutput, then family 1 with the structured ones."""
    B, C, H, W = shape
    nOut, oH, oW = L.out_shape(H, W, *CORR)
    for fam in fams:
        a, b = L.family_inputs(fam, shape, dtype, seed)
        yield a, b, L.grad_output("normal", (B, nOut, oH, oW), dtype, seed + fam), f"{shape} family {fam}"
    a, b = L.family_inputs(1, shape, dtype, seed)
    for kind in grads:
        yield a, b, L.grad_output(kind, (B, nOut, oH, oW), dtype, seed), f"{shape} family 1, gradOutput {kind}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("case", BWD_NARROW)
def test_backward_matrix_kernel(dev, case, dtype):
    for a, b, go, what in _bwd_runs(case, dtype, sum(case)):
        _check_backward(dev, a, b, go, CORR, dtype, "matrix", what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("case", BWD_WIDE)
def test_backward_widened(dev, case, dtype):
    for a, b, go, what in _bwd_runs(case, dtype, sum(case)):
        _check_backward(dev, a, b, go, CORR, dtype, "widened", what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("gen", GEN_BWD, ids=["C96", "k3"])
def test_backward_general_kernel(dev, gen, dtype):
    params, shape, fams = gen
    B, C, H, W = shape
    nOut, oH, oW = L.out_shape(H, W, *params)
    for fam in fams:
        a, b = L.family_inputs(fam, shape, dtype, seed=sum(shape))
        go = L.grad_output("normal", (B, nOut, oH, oW), dtype, sum(shape) + fam)
        _check_backward(dev, a, b, go, params, dtype, "general", f"{params} {shape} family {fam}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("case", [(2, 192, 46, 56), (1, 192, 48, 72)])
def test_fused_backward(dev, case, dtype):
    """backward_fused against the float64 backward of the masked gradient (LeakyReLU's derivative taken from the stored output,
    applied in T as autograd does), and bit-identical to the unfused backward on that gradient (narrow: the matrix kernel; wide:
    the widened path)."""
    import correlation_cuda
    import fn2_capi
    B, C, H, W = case
    a, b = L.family_inputs(3, case, dtype, seed=sum(case))
    ad, bd = a.to(dev), b.to(dev)
    buf = torch.zeros((B, 8 + 441, H, W), dtype=dtype, device=dev)
    fn2_capi.correlation_forward_fused(ad, bd, buf, 8, SLOPE, *CORR)
    gbuf = L.grad_output("normal", tuple(buf.shape), dtype, sum(case)).to(dev)
    masked = torch.ops.aten.leaky_relu_backward(gbuf[:, 8:].contiguous(), buf[:, 8:].contiguous(), SLOPE, True)
    kernel = "matrix" if W <= 64 else "widened"
    if kernel == "matrix":
        f1, f2 = fn2_capi.correlation_backward_fused(ad, bd, buf, gbuf, 8, SLOPE, *CORR)
        u1, u2 = fn2_capi.correlation_backward(ad, bd, masked, *CORR)
    else:
        f1, f2 = _nan(a.shape, dtype, dev), _nan(a.shape, dtype, dev)
        correlation_cuda.backward_fused(ad, bd, buf, gbuf, 8, SLOPE, f1, f2, *CORR)
        u1, u2 = correlation_cuda.backward_alloc(ad, bd, masked, *CORR, 1)
    assert torch.equal(f1, u1) and torch.equal(f2, u2)
    for name, got, (ref, delta) in zip(("grad_input1", "grad_input2"), (f1, f2), _bwd_ref(ad, bd, masked, CORR, kernel)):
        assert not torch.isnan(got).any()
        lo, hi = L.bracket(ref, delta, dtype)
        L.check_bracket(got, lo, hi, f"{case} fused {name}")


# ------------------------------------------------------------------ ChannelNorm
CN_SHAPES = [(2, 3, 16, 24), (1, 2, 7, 9), (3, 5, 6, 10), (8, 3, 384, 512), (8, 2, 384, 512)]   # HW % 8 != 0: the scalar kernels


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("shape", CN_SHAPES)
def test_channelnorm(dev, shape, dtype):
    """Forward: sqrt of an fp32 sum of squares (half squares rounded to half, bf16 squares exact), one rounding.  Backward:
    go * x / (out + 1e-9), with a contiguous gradOutput and a strided one (a window of a wider tensor), input families 1-3."""
    import channelnorm_cuda
    B, C, H, W = shape
    for fam in (1, 2, 3):
        x, _ = L.family_inputs(fam, shape, dtype, seed=C * H + W)
        xd = x.to(dev)
        out = _nan((B, 1, H, W), dtype, dev)
        channelnorm_cuda.forward(xd, out, 2)
        assert not torch.isnan(out).any()
        lo, hi = L.chnorm_fwd_bracket(xd, dtype)
        L.check_bracket(out, lo, hi, f"{shape} family {fam} forward")
        gfull = L.grad_output("normal", (B, 1, H, W + 3), dtype, fam).to(dev)
        for go in (gfull[..., 1:W + 1].contiguous(), gfull[..., 1:W + 1]):
            gin = _nan(shape, dtype, dev)
            channelnorm_cuda.backward(xd, out, go, gin, 2)
            assert not torch.isnan(gin).any()
            lo, hi = L.chnorm_bwd_bracket(xd, out, go)
            L.check_bracket(gin, lo, hi, f"{shape} family {fam} backward, gradOutput contiguous={go.is_contiguous()}")
