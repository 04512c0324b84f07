"""bfloat16 tensors through the layers (FN2_BF16): Correlation and ChannelNorm on native bf16 kernels (the correlation on
v_mfma_f32_16x16x32_bf16), Resample2d and MultiScale widened to fp32 around their kernels, and the harness models under
torch.autocast(dtype=torch.bfloat16).  Inputs are seeded and bf16-rounded; references are the oracle (or the fp32 kernels) on
those values widened to fp32; outputs are prefilled with NaN so that unwritten elements show."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import max_abs

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CORR = (20, 1, 20, 1, 2)                   # FlowNetC's cost volume (FlowNetC.py:28)
FWD_CASES = [(1, 128, 6, 8), (2, 128, 16, 24), (1, 256, 22, 56), (1, 128, 46, 64), (3, 128, 2, 16), (2, 256, 48, 64),
             (1, 128, 8, 72), (2, 128, 10, 96), (1, 256, 56, 128), (1, 128, 4, 200), (3, 128, 6, 104)]   # W > 64: column windows


def _bf(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(BF)


@pytest.mark.parametrize("case", FWD_CASES)
def test_bf16_correlation_forward(dev, oracle, case):
    """AUTO = the bf16 matrix kernels (narrow, column-window): products exact in fp32, fp32 sums, one rounding to bf16 -- within
    2^-8 of the output scale; DIRECT (the general kernel) agrees; the fused LeakyReLU + concat store touches only its slice."""
    import fn2_capi
    B, C, H, W = case
    rng = np.random.default_rng(B * 1000 + C + H + W + 77)
    a, b = _bf(rng, (B, C, H, W)), _bf(rng, (B, C, H, W))
    ad, bd = a.to(dev), b.to(dev)
    ref = oracle.corr_fwd(a.float().numpy(), b.float().numpy(), *CORR)
    out = torch.full((B, 441, H, W), float("nan"), dtype=BF, device=dev)
    fn2_capi.correlation_forward(ad, bd, *CORR, out=out)                                # AUTO
    got = out.float().cpu().numpy()
    assert np.isfinite(got).all(), "unwritten output elements"
    scale = float(np.abs(ref).max())
    assert max_abs(got, ref) <= 2.0 ** -8 * scale + 1e-6, (max_abs(got, ref), scale)
    direct = fn2_capi.correlation_forward(ad, bd, *CORR, algo=fn2_capi.FN2_CORR_DIRECT)
    assert float((out.float() - direct.float()).abs().max()) <= 2.0 ** -7 * scale
    sel = fn2_capi.correlation_forward(ad, bd, *CORR, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
    assert torch.equal(sel, out)                                                         # the explicit selector: same kernel
    # fused LeakyReLU 0.1 + store into a concat slice; the channels around it stay untouched
    buf = torch.full((B, 8 + 441 + 3, H, W), 7.0, dtype=BF, device=dev)
    fn2_capi.correlation_forward_fused(ad, bd, buf, 8, 0.1, *CORR)
    assert (buf[:, :8] == 7.0).all() and (buf[:, 8 + 441:] == 7.0).all()
    want = F.leaky_relu(out.float(), 0.1)
    # one rounding of leaky(acc) against leaky applied to the rounded acc: within one bf16 ulp (<= 2^-7 |x|)
    assert bool(((buf[:, 8:8 + 441].float() - want).abs() <= 2.0 ** -7 * want.abs() + 1e-30).all())


def test_bf16_correlation_forward_general_kernel(dev, oracle):
    import fn2_capi
    rng = np.random.default_rng(5)
    a, b = _bf(rng, (2, 32, 16, 20)), _bf(rng, (2, 32, 16, 20))
    for params in [(3, 3, 4, 2, 2), (3, 3, 4, 1, 2), (2, 1, 4, 2, 1)]:                  # k = 3, stride1 = 2, C = 32
        ref = oracle.corr_fwd(a.float().numpy(), b.float().numpy(), *params)
        got = fn2_capi.correlation_forward(a.to(dev), b.to(dev), *params).float().cpu().numpy()
        assert np.isfinite(got).all()
        assert max_abs(got, ref) <= 2.0 ** -8 * float(np.abs(ref).max()) + 1e-6, params


@pytest.mark.parametrize("case", [(2, 128, 16, 24), (2, 256, 48, 64), (1, 64, 6, 8), (1, 128, 8, 72), (1, 64, 10, 96)])
def test_bf16_correlation_backward(dev, oracle, case):
    """Narrow maps: the bf16 matrix kernel; wider than 64 px: the binding's widened path (fp32 column-window kernel, one rounding)."""
    import correlation_cuda
    import fn2_capi
    B, C, H, W = case
    rng = np.random.default_rng(B * 1000 + C + H + W + 9)
    a, b, go = _bf(rng, (B, C, H, W)), _bf(rng, (B, C, H, W)), _bf(rng, (B, 441, H, W))
    ad, bd, gd = a.to(dev), b.to(dev), go.to(dev)
    r1, r2 = oracle.corr_bwd(a.float().numpy(), b.float().numpy(), go.float().numpy(), *CORR)
    if W <= 64:
        g1 = torch.full((B, C, H, W), float("nan"), dtype=BF, device=dev)
        g2 = torch.full((B, C, H, W), float("nan"), dtype=BF, device=dev)
        fn2_capi.correlation_backward(ad, bd, gd, *CORR, out=(g1, g2))                   # AUTO
        s1, s2 = fn2_capi.correlation_backward(ad, bd, gd, *CORR, algo=fn2_capi.FN2_CORR_MFMA_F16X2)
        assert torch.equal(s1, g1) and torch.equal(s2, g2)
    else:
        g1, g2 = correlation_cuda.backward_alloc(ad, bd, gd, *CORR, 1)
    for got, ref in ((g1, r1), (g2, r2)):
        assert got.dtype == BF
        n = got.float().cpu().numpy()
        assert np.isfinite(n).all(), "unwritten gradient elements"
        assert max_abs(n, ref) <= 2.0 ** -8 * float(np.abs(ref).max()) + 1e-6


def test_bf16_correlation_backward_general_kernel(dev, oracle):
    import fn2_capi
    rng = np.random.default_rng(6)
    params = (3, 3, 4, 1, 2)                                                              # k = 3, C = 32, stride1 = 1
    a, b = _bf(rng, (2, 32, 12, 14)), _bf(rng, (2, 32, 12, 14))
    nout, oh, ow = fn2_capi.correlation_output_shape(12, 14, *params)
    go = _bf(rng, (2, nout, oh, ow))
    r1, r2 = oracle.corr_bwd(a.float().numpy(), b.float().numpy(), go.float().numpy(), *params)
    g1, g2 = fn2_capi.correlation_backward(a.to(dev), b.to(dev), go.to(dev), *params)
    for got, ref in ((g1, r1), (g2, r2)):
        assert max_abs(got.float().cpu().numpy(), ref) <= 2.0 ** -8 * float(np.abs(ref).max()) + 1e-6


@pytest.mark.parametrize("case", [(2, 128, 16, 24), (1, 64, 8, 72)])
def test_bf16_correlation_fused_backward_bit_identical(dev, case):
    """backward_fused = autograd's bf16 leaky_relu_backward (fp32 product, one rounding) followed by the unfused backward, bit for bit
    (narrow: the C ABI; wide: the binding's widened path)."""
    import correlation_cuda
    import fn2_capi
    B, C, H, W = case
    rng = np.random.default_rng(31 + W)
    ad, bd = _bf(rng, (B, C, H, W)).to(dev), _bf(rng, (B, C, H, W)).to(dev)
    buf = torch.full((B, 8 + 441, H, W), 3.0, dtype=BF, device=dev)
    fn2_capi.correlation_forward_fused(ad, bd, buf, 8, 0.1, *CORR)
    gbuf = _bf(rng, tuple(buf.shape)).to(dev)
    masked = torch.ops.aten.leaky_relu_backward(gbuf[:, 8:].contiguous(), buf[:, 8:].contiguous(), 0.1, True)
    if W <= 64:
        f1, f2 = fn2_capi.correlation_backward_fused(ad, bd, buf, gbuf, 8, 0.1, *CORR)
        u1, u2 = fn2_capi.correlation_backward(ad, bd, masked, *CORR)
    else:
        f1, f2 = torch.empty(0, dtype=BF, device=dev), torch.empty(0, dtype=BF, device=dev)
        correlation_cuda.backward_fused(ad, bd, buf, gbuf, 8, 0.1, f1, f2, *CORR)
        u1, u2 = correlation_cuda.backward_alloc(ad, bd, masked, *CORR, 1)
    assert torch.equal(f1, u1) and torch.equal(f2, u2)


def test_bf16_correlation_non_finite_inputs(dev, oracle):
    """inf / nan are operands like any other: exactly the outputs whose sums include them are non-finite (forward: against the oracle;
    backward: against the general fp32 kernel, which the fp32 suite pins to the oracle)."""
    import fn2_capi
    rng = np.random.default_rng(44)
    a, b = _bf(rng, (1, 128, 8, 16)), _bf(rng, (1, 128, 8, 16))
    # (non-finite values in input2 only for the forward: an inf in input1 that meets the zero padding of input2 is inf * 0 = nan in
    #  the matrix kernels' zero-filled padding, 0 in the oracle -- as for half tensors)
    b[0, 3, 2, 2] = float("inf"); b[0, 5, 4, 4] = float("nan"); b[0, 9, 6, 11] = -float("inf")
    out = fn2_capi.correlation_forward(a.to(dev), b.to(dev), *CORR).float().cpu().numpy()
    ref = oracle.corr_fwd(a.float().numpy(), b.float().numpy(), *CORR)
    assert (~np.isfinite(ref)).sum() > 0
    assert np.array_equal(np.isfinite(out), np.isfinite(ref)) and np.array_equal(np.isnan(out), np.isnan(ref))
    fin = np.isfinite(ref)
    assert max_abs(out[fin], ref[fin]) <= 2.0 ** -8 * float(np.abs(ref[fin]).max()) + 1e-6
    go = _bf(rng, (1, 441, 8, 16))
    a2, b2, g2 = a.clone(), _bf(rng, (1, 128, 8, 16)), go.clone()
    a2[0, 3, 4, 11] = float("inf"); b2[0, 7, 1, 3] = float("nan"); g2[0, 220, 0, 3] = float("inf")
    n1, n2 = fn2_capi.correlation_backward(a2.to(dev), b2.to(dev), g2.to(dev), *CORR)
    f1, f2 = fn2_capi.correlation_backward(a2.float().to(dev), b2.float().to(dev), g2.float().to(dev), *CORR,
                                           algo=fn2_capi.FN2_CORR_DIRECT)
    for got, ref in ((n1, f1), (n2, f2)):
        assert int((~torch.isfinite(ref)).sum()) > 0
        assert torch.equal(torch.isfinite(got), torch.isfinite(ref)) and torch.equal(torch.isnan(got), torch.isnan(ref))
        fin = torch.isfinite(ref)
        assert float((got.float() - ref)[fin].abs().max()) <= 2.0 ** -8 * float(ref[fin].abs().max()) + 1e-6


# v_mfma_f32_16x16x32_bf16 keeps subnormal bf16 operands (measured on an MI355X by the test below; documented at FN2_BF16 in
# include/flownet2_hip.h).
MFMA_BF16_KEEPS_SUBNORMALS = True


def test_bf16_mfma_subnormal_operands(dev):
    """A subnormal bf16 operand (2^-130; bf16's smallest normal is 2^-126) times 2^100 is 2^-30: the product the matrix kernel
    delivers either holds it (subnormals kept) or not (flushed).  The measured behaviour is pinned here and documented at FN2_BF16."""
    import fn2_capi
    B, C, H, W = 1, 128, 6, 8
    a = torch.zeros(B, C, H, W, dtype=BF)
    b = torch.zeros(B, C, H, W, dtype=BF)
    a[:, 0] = 2.0 ** -130
    b[:, 0] = 2.0 ** 100
    assert float(a[0, 0, 0, 0]) == 2.0 ** -130 and float(a[0, 0, 0, 0]) < torch.finfo(BF).tiny
    out = fn2_capi.correlation_forward(a.to(dev), b.to(dev), *CORR).float().cpu()
    centre = out[:, 220]                                                                   # displacement (0, 0): every pixel
    want = 2.0 ** -30 / C
    kept = bool((centre == want).all())
    flushed = bool((centre == 0).all())
    print(f"bf16 MFMA subnormal operand: kept={kept} flushed={flushed}")
    assert kept != flushed, "neither exact nor flushed: " + str(centre.unique())
    assert kept == MFMA_BF16_KEEPS_SUBNORMALS


@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 5, 17, 19), (8, 3, 384, 512)])
def test_bf16_channelnorm(dev, oracle, shape):
    import channelnorm_cuda
    from networks.channelnorm_package.channelnorm import ChannelNorm
    B, C, H, W = shape
    rng = np.random.default_rng(C * H + W)
    x = _bf(rng, shape)
    xd = x.to(dev)
    out = ChannelNorm()(xd)
    assert out.dtype == BF
    ref = oracle.chnorm_fwd(x.float().numpy())
    got = out.float().cpu().numpy()
    assert (np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + 1e-30).all()
    # backward with a strided gradOutput (a window of a wider tensor), against the oracle on the same values
    gfull = _bf(rng, (B, 1, H, W + 3)).to(dev)
    go = gfull[..., 1:W + 1]
    assert not go.is_contiguous()
    gin = torch.full(shape, float("nan"), dtype=BF, device=dev)
    channelnorm_cuda.backward(xd, out, go, gin, 2)
    rg = oracle.chnorm_bwd(x.float().numpy(), got, go.float().cpu().numpy())
    g = gin.float().cpu().numpy()
    assert np.isfinite(g).all()
    assert (np.abs(g - rg) <= 2.0 ** -8 * np.abs(rg) + 1e-30).all()


def test_bf16_resample2d(dev):
    import resample2d_cuda
    from networks.resample2d_package.resample2d import Resample2d
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(2, 3, 32, 48, generator=g) - 0.5).to(BF)
    f = (torch.randn(2, 2, 32, 48, generator=g) * 3).to(BF)
    go = torch.randn(2, 3, 32, 48, generator=g).to(BF).to(dev)
    xd, fd = x.to(dev).requires_grad_(True), f.to(dev).requires_grad_(True)
    out = Resample2d()(xd, fd)
    want = resample2d_cuda.forward_alloc(x.float().to(dev), f.float().to(dev), 1, True)
    assert out.dtype == BF and torch.equal(out, want.to(BF))
    out.backward(go)
    gi, gf = resample2d_cuda.backward_alloc(x.float().to(dev), f.float().to(dev), go.float(), 1, True)
    assert fd.grad.dtype == BF and torch.equal(fd.grad, gf.to(BF))
    # grad_img: fp32 atomics in an unspecified order, one rounding: within one bf16 ulp
    assert bool(((xd.grad.float() - gi).abs() <= 2.0 ** -7 * gi.abs() + 1e-6 * float(gi.abs().max())).all())
    with pytest.raises(RuntimeError, match="float32"):
        resample2d_cuda.forward_alloc(x.half().to(dev), f.half().to(dev), 1, True)


def test_bf16_warp_diff_norm_modules(dev):
    """WarpDiffNormCat / WarpDiffNorm on bf16 tensors: the fused fp32 kernels on the widened values, each result rounded once."""
    from networks.resample2d_package.resample2d import WarpDiffNorm, WarpDiffNormCat
    g = torch.Generator().manual_seed(12)
    x = (torch.rand(2, 6, 32, 48, generator=g) - 0.5).to(BF).to(dev)
    f = (torch.randn(2, 2, 32, 48, generator=g) * 3).to(BF).to(dev)
    for mod in (WarpDiffNormCat(div_flow=20.0), WarpDiffNorm()):
        fb = f.clone().requires_grad_(True)
        ff = f.float().requires_grad_(True)
        out = mod(x, fb)
        want = mod(x.float(), ff)
        assert out.dtype == BF and torch.equal(out, want.to(BF))
        go = torch.randn(out.shape, generator=g).to(BF).to(dev)
        out.backward(go)
        want.backward(go.float())
        assert fb.grad.dtype == BF and torch.equal(fb.grad, ff.grad.to(BF))


def test_bf16_multiscale_loss(dev):
    from losses_fused import MultiScaleL1
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 128, 192
    target = (torch.randn(B, 2, H, W, generator=g) * 5).to(dev)
    crit = MultiScaleL1()
    for dt in (BF, torch.float16):
        preds = [torch.randn(B, 2, H // k, W // k, generator=g).to(dt).to(dev).requires_grad_(True) for k in (4, 8, 16, 32, 64)]
        wide = [p.detach().float().requires_grad_(True) for p in preds]
        loss, epe = crit(preds, target)
        loss_f, epe_f = crit(wide, target)
        assert loss.dtype == torch.float32 and torch.equal(loss, loss_f) and torch.equal(epe, epe_f)
        loss.backward()
        loss_f.backward()
        for p, q in zip(preds, wide):
            assert p.grad.dtype == dt and torch.equal(p.grad, q.grad.to(dt))
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        crit([torch.zeros(B, 2, H // k, W // k, dtype=torch.float64, device=dev) for k in (4, 8, 16, 32, 64)], target)


def test_bf16_autocast_flownetc_style_module(dev):
    """conv -> Correlation -> LeakyReLU -> cat, as FlowNetC.py writes it, under bf16 autocast: forward and backward run, the cost
    volume and the gradients reaching the features are bf16."""
    from networks.correlation_package.correlation import Correlation

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv3 = torch.nn.Conv2d(16, 128, 3, 1, 1)
            self.conv_redir = torch.nn.Conv2d(128, 32, 1)
            self.corr = Correlation(pad_size=20, kernel_size=1, max_displacement=20, stride1=1, stride2=2, corr_multiply=1)
            self.act = torch.nn.LeakyReLU(0.1, inplace=True)

        def forward(self, x1, x2):
            a, b = self.conv3(x1), self.conv3(x2)
            a.retain_grad(); b.retain_grad()
            corr = self.act(self.corr(a, b))
            self.seen = (a, b, corr)
            return torch.cat((self.conv_redir(a), corr), 1)

    torch.manual_seed(0)
    net = Net().to(dev)
    x1, x2 = torch.randn(2, 16, 16, 24, device=dev), torch.randn(2, 16, 16, 24, device=dev)
    with torch.autocast("cuda", dtype=BF):
        y = net(x1, x2)
        loss = y.float().square().mean()
    loss.backward()
    a, b, corr = net.seen
    assert corr.dtype == BF and y.dtype == BF and tuple(corr.shape) == (2, 441, 16, 24)
    assert a.grad.dtype == BF and b.grad.dtype == BF
    assert bool(torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all() and torch.isfinite(net.conv3.weight.grad).all())


def _rel_rms(x, ref):
    x, ref = x.float(), ref.float()
    return float((x - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


# bf16 autocast against fp32 on the same weights, relative RMS of the flow.  Measured on an MI355X: FlowNet2C training flow2
# 2.9e-3, FlowNet2 inference 2.4e-2; bounds with headroom over those.
REL_RMS_BOUND_FLOWNET2C = 1e-2
REL_RMS_BOUND_FLOWNET2 = 5e-2


def test_bf16_autocast_harness_models(dev):
    """FlowNet2C training step and FlowNet2 inference under bf16 autocast, bs 2 @ 128x192, the same weights as the fp32 run."""
    from harness.flownet2 import FlowNet2
    from harness.flownet2c import FlowNet2C
    from harness.train import synthetic_batch
    from losses_fused import MultiScaleL1
    inputs, target = synthetic_batch(2, 128, 192, dev, seed=4)
    torch.manual_seed(2)
    model = FlowNet2C().to(dev).train()
    crit = MultiScaleL1()
    flows32 = model(inputs)
    crit(flows32, target)[0].backward()
    g32 = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=BF):
        flows16 = model(inputs)
        loss16, epe16 = crit(flows16, target)
    loss16.backward()
    assert all(bool(torch.isfinite(f).all()) for f in flows16) and bool(torch.isfinite(loss16)) and bool(torch.isfinite(epe16))
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    r = _rel_rms(flows16[0], flows32[0])
    rg = _rel_rms(dict(model.named_parameters())["conv3_1.0.weight"].grad, g32["conv3_1.0.weight"])
    print(f"FlowNet2C bf16 autocast: flow2 rel RMS {r:.3e}, conv3_1 weight-gradient rel RMS {rg:.3e}")
    assert r <= REL_RMS_BOUND_FLOWNET2C, r
    # FlowNet2 inference
    torch.manual_seed(3)
    net2 = FlowNet2().to(dev).eval()
    with torch.no_grad():
        out32 = net2(inputs)
        with torch.autocast("cuda", dtype=BF):
            out16 = net2(inputs)
    assert bool(torch.isfinite(out16).all())
    r2 = _rel_rms(out16, out32)
    print(f"FlowNet2 bf16 autocast inference: flow rel RMS {r2:.3e}")
    assert r2 <= REL_RMS_BOUND_FLOWNET2, r2


def test_bf16_trainer_autocast(dev):
    from harness.train import Trainer, synthetic_batch
    inputs, target = synthetic_batch(2, 128, 192, dev, seed=5)
    tr = Trainer(dev, autocast_dtype=BF)
    loss, epe = tr.train_step(inputs, target)
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss)) and bool(torch.isfinite(epe))
    assert all(p.dtype == torch.float32 and bool(torch.isfinite(p).all()) for p in tr.model.parameters())
