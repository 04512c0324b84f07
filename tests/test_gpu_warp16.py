"""The fused warp rows on half and bfloat16 tensors (fn2_warp_diff_norm*_16), bit for bit.

Contract (include/flownet2_hip.h): every element a 16-bit entry point writes has the bits of the float32 entry point run on the exactly
widened inputs, its float32 result rounded to the 16-bit type once (round to nearest even, overflow -> inf, subnormals kept, NaN stays
NaN).  The backward passes recompute the warp and the norm; their reference is the float32 backward fed the widened pair, flow and
gradient AND the float32 forward's own (unrounded) output.

Reference in this file = the unchanged float32 entry points through fn2_capi on `.float()` inputs, narrowed ON THE CPU
(`ref.cpu().to(dtype)`: IEEE round to nearest even with subnormals, independent of the device's convert instructions).  Comparison on
the raw 16-bit patterns; NaN positions are compared as a mask.  Zero mismatches allowed -- the one tolerance is the pair-gradient case
(float32 atomics, order unspecified): one 16-bit ulp, the bound of tests/test_gpu_bf16.py::test_bf16_resample2d.

Every case runs through three levels: the C ABI (fn2_capi), the pybind functions (resample2d_cuda) and the nn.Modules under autograd."""
import threading

import pytest
import torch

import fn2_capi

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
ULP1 = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}      # the type's ulp at 1
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ comparison and references
def assert_bits(got, ref32, dt, what):
    """got (16-bit, device) == ref32 (float32, device) narrowed on the CPU, bit for bit; NaNs compared as a mask"""
    assert got.dtype == dt and got.shape == ref32.shape, (what, got.dtype, got.shape, ref32.shape)
    g, w = got.detach().cpu().contiguous(), ref32.detach().cpu().to(dt).contiguous()
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert torch.equal(gn, wn), (what, "NaN positions differ", int((gn != wn).sum()), "of", g.numel())
    bad = (g.view(torch.int16) != w.view(torch.int16)) & ~gn
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError((what, "mismatching elements", n, "of", g.numel(), "first at", i, float(g.flatten()[i]), float(w.flatten()[i])))


def ref_cat(pair, flow, div, bilinear):
    return fn2_capi.warp_diff_norm_cat(pair.float().contiguous(), flow.float().contiguous(), div, bilinear)


def ref_cat_bwd(pair, flow, gcat, div, bilinear):
    p, f = pair.float().contiguous(), flow.float().contiguous()
    out32 = fn2_capi.warp_diff_norm_cat(p, f, div, bilinear)          # the float32 forward's own output, unrounded
    return fn2_capi.warp_diff_norm_cat_backward(p, f, out32, gcat.float().contiguous(), div, bilinear, want_grad_pair=False)[1]


def ref_norm(pair, flow, bilinear):
    return fn2_capi.warp_diff_norm(pair.float().contiguous(), flow.float().contiguous(), bilinear)


def ref_norm_bwd(pair, flow, gn, bilinear):
    p, f = pair.float().contiguous(), flow.float().contiguous()
    return fn2_capi.warp_diff_norm_backward(p, f, fn2_capi.warp_diff_norm(p, f, bilinear), gn.float().contiguous(), bilinear)


def check_all_levels(pair, flow, gcat, gn, div=20.0, bilinear=True, what=""):
    """both rows, forward and flow-gradient backward, through the C ABI, the pybind functions and the modules"""
    import resample2d_cuda
    from networks.resample2d_package.resample2d import WarpDiffNorm, WarpDiffNormCat
    dt = pair.dtype
    B, C2, H, W = pair.shape
    C = C2 // 2
    r_cat, r_norm = ref_cat(pair, flow, div, bilinear), ref_norm(pair, flow, bilinear)
    r_gcat, r_gnorm = ref_cat_bwd(pair, flow, gcat, div, bilinear), ref_norm_bwd(pair, flow, gn, bilinear)
    # 1. C ABI (outputs prefilled with NaN by the fn2_capi wrappers: an unwritten element shows as a NaN the reference lacks)
    assert_bits(fn2_capi.warp_diff_norm_cat_16(pair, flow, div, bilinear), r_cat, dt, (what, "capi cat"))
    assert_bits(fn2_capi.warp_diff_norm_16(pair, flow, bilinear), r_norm, dt, (what, "capi norm"))
    assert_bits(fn2_capi.warp_diff_norm_cat_backward_16(pair, flow, gcat, div, bilinear), r_gcat, dt, (what, "capi cat bwd"))
    assert_bits(fn2_capi.warp_diff_norm_backward_16(pair, flow, gn, bilinear), r_gnorm, dt, (what, "capi norm bwd"))
    # 2. pybind
    out = torch.full((B, 3 * C + 3, H, W), NAN, dtype=dt, device=pair.device)
    assert resample2d_cuda.warp_diff_norm_cat(pair, flow, out, div, bilinear) == 1
    assert_bits(out, r_cat, dt, (what, "pybind cat"))
    assert_bits(resample2d_cuda.warp_diff_norm(pair, flow, bilinear), r_norm, dt, (what, "pybind norm"))
    none, gflow = pair.new_empty(0), torch.full_like(flow, NAN)
    assert resample2d_cuda.warp_diff_norm_cat_backward(pair, flow, none, gcat, none, gflow, div, bilinear) == 1
    assert_bits(gflow, r_gcat, dt, (what, "pybind cat bwd"))
    assert_bits(resample2d_cuda.warp_diff_norm_backward(pair, flow, none, gn, bilinear), r_gnorm, dt, (what, "pybind norm bwd"))
    # 3. modules under autograd (the C++ nodes) and the Python Function twins
    for cat_apply, norm_apply, lvl in ((lambda x, f: WarpDiffNormCat(div, bilinear)(x, f), lambda x, f: WarpDiffNorm(bilinear)(x, f), "module"),
                                       (lambda x, f: _PyCat.apply(x, f, div, bilinear), lambda x, f: _PyNorm.apply(x, f, bilinear), "python twin")):
        f1 = flow.clone().requires_grad_(True)
        o = cat_apply(pair, f1)
        assert o.dtype == dt and tuple(o.shape) == (B, 3 * C + 3, H, W)
        assert_bits(o, r_cat, dt, (what, lvl, "cat"))
        if o.numel():
            o.backward(gcat)
            assert_bits(f1.grad, r_gcat, dt, (what, lvl, "cat bwd"))
        f2 = flow.clone().requires_grad_(True)
        n = norm_apply(pair, f2)
        assert n.dtype == dt and tuple(n.shape) == (B, 1, H, W)
        assert_bits(n, r_norm, dt, (what, lvl, "norm"))
        if n.numel():
            n.backward(gn)
            assert_bits(f2.grad, r_gnorm, dt, (what, lvl, "norm bwd"))


class _Twin:
    """torch.autograd.Function.apply over the Python forward / backward twins (the classes' own `apply` is the C++ node)"""
    def __init__(self, name):
        self.name = name

    def apply(self, *a):
        from networks.resample2d_package import resample2d as m
        cls = getattr(m, self.name)
        return super(cls, cls).apply(*a)


_PyCat, _PyNorm = _Twin("WarpDiffNormCatFunction"), _Twin("WarpDiffNormFunction")


# ------------------------------------------------------------------------------------------------ inputs
def rnd(g, shape, scale=1.0):
    return torch.randn(shape, generator=g) * scale


def make_flow(kind, g, B, H, W):
    if kind == "noise":          # sub-pixel noise, a few pixels
        return rnd(g, (B, 2, H, W), 3.0)
    if kind == "translate":      # whole tiles moved beyond the 16-px window radius: the global-gather branch
        f = rnd(g, (B, 2, H, W), 0.7)
        f[:, 0] += 37.25
        f[:, 1] -= 21.5
        return f
    if kind == "far":            # far outside the image: clamping
        return rnd(g, (B, 2, H, W), 2000.0)
    if kind == "grid":           # exact integers and exact .5 (floor, and the tie of the nearest mode)
        return torch.randint(-6, 7, (B, 2, H, W), generator=g).float() * 0.5
    raise ValueError(kind)


def make_case(dt, dev, shape, kind, seed, grad="normal", offset=False):
    B, C2, H, W = shape
    g = torch.Generator().manual_seed(seed)
    pair, flow = rnd(g, shape, 0.5), make_flow(kind, g, B, H, W)
    gcat, gn = rnd(g, (B, C2 + C2 // 2 + 3, H, W)), rnd(g, (B, 1, H, W))
    if grad == "sparse":         # one plane non-zero
        keep = gcat[:, C2 + 1].clone()
        gcat.zero_()
        gcat[:, C2 + 1] = keep
        gn[:, :, ::2] = 0
    elif grad == "zero":
        gcat.zero_(); gn.zero_()

    def put(t):
        t = t.to(dt)
        if not offset:
            return t.to(dev).contiguous()
        flat = torch.zeros(t.numel() + 1, dtype=dt, device=dev)      # planes 2-byte but not 16-byte aligned: the fallback
        v = flat[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 4 == 2 and v.is_contiguous()
        return v
    return put(pair), put(flow), put(gcat), put(gn)


BIG, RAGGED = (8, 6, 384, 512), (2, 6, 50, 104)
CASES = [
    # (shape, flow kind, bilinear, gradient, offset)
    (BIG, "noise", True, "normal", False),          # the graded size, tiled path
    (BIG, "translate", True, "normal", False),      # ... every sample outside the LDS window
    (RAGGED, "noise", True, "normal", False),       # ragged tiles
    (RAGGED, "translate", True, "sparse", False),
    (RAGGED, "far", True, "normal", False),
    (RAGGED, "grid", True, "normal", False),
    (RAGGED, "grid", False, "normal", False),       # nearest, ties at .5
    (RAGGED, "noise", False, "normal", False),
    (RAGGED, "noise", True, "zero", False),
    ((2, 6, 40, 100), "noise", True, "normal", False),     # W % 8 != 0
    ((2, 6, 12, 64), "noise", True, "normal", False),      # H < 16
    ((2, 4, 33, 40), "noise", True, "sparse", False),      # C = 2
    ((1, 10, 24, 48), "translate", True, "normal", False), # C = 5
    ((1, 10, 24, 48), "grid", False, "normal", False),
    (RAGGED, "noise", True, "normal", True),               # 2-byte aligned planes
    (RAGGED, "grid", False, "sparse", True),
    ((0, 6, 32, 64), "noise", True, "normal", False),      # B = 0
]


@pytest.mark.parametrize("dt", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%s-%s%s" % ("x".join(map(str, c[0])), c[1], "bil" if c[2] else "nearest", c[3], "-off" if c[4] else ""))
def test_rows_bit_for_bit(dev, dt, case):
    shape, kind, bilinear, grad, offset = case
    pair, flow, gcat, gn = make_case(dt, dev, shape, kind, 1000 + CASES.index(case), grad, offset)
    check_all_levels(pair, flow, gcat, gn, 20.0, bilinear, case)


@pytest.mark.parametrize("dt", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("shape", [(1, 6, 32, 64), (1, 6, 9, 20)], ids=["tiled", "fallback"])
def test_rounding_ties_round_once_to_even(dev, dt, shape):
    """flow (0.5, 0): alpha = 0.5, beta = 0, the warp is the exact mean of two horizontal neighbours.  Neighbours 1 and 1 + u (u = the
    type's ulp at 1) give exactly 1 + u/2, a tie that must round to 1 (even); 1 + u and 1 + 2u give 1 + 3u/2, which must round to
    1 + 2u.  A kernel that truncates, rounds half up, or rounds twice fails here."""
    B, C2, H, W = shape
    u = ULP1[dt]
    row = torch.tensor([1.0, 1.0 + u, 1.0 + 2 * u, 1.0 + u]).repeat(W // 4)
    pair = torch.zeros(shape)
    pair[:, 3:] = row
    flow = torch.zeros(B, 2, H, W)
    flow[:, 0] = 0.5
    pair, flow = pair.to(dt).to(dev), flow.to(dt).to(dev)
    assert torch.equal(pair[0, 3, 0, :4].float().cpu(), row[:4])              # the values are exact in the 16-bit type
    out = fn2_capi.warp_diff_norm_cat_16(pair, flow, 20.0, True)
    warped = out[:, 6:9].float().cpu()
    want = torch.tensor([1.0, 1.0 + 2 * u, 1.0 + 2 * u, 1.0]).repeat(W // 4)
    assert bool((warped[..., :W - 1] == want[:W - 1]).all())
    g = torch.Generator().manual_seed(5)
    check_all_levels(pair, flow, rnd(g, (B, 12, H, W)).to(dt).to(dev), rnd(g, (B, 1, H, W)).to(dt).to(dev), 20.0, True, "ties")


@pytest.mark.parametrize("shape", [(2, 6, 32, 64), (2, 6, 10, 24)], ids=["tiled", "fallback"])
def test_half_overflow_and_subnormal_norms(dev, shape):
    """half only: image values up to 6e4, so that some norms (up to 1.2e5 * sqrt(3)) overflow to inf, and differences of a few half
    subnormal steps (2^-24), so that the norm itself is a half subnormal and has to be rounded on the subnormal grid."""
    dt = torch.float16
    B, C2, H, W = shape
    g = torch.Generator().manual_seed(6)
    pair = torch.zeros(shape)
    pair[0, :3] = torch.rand((3, H, W), generator=g) * 6e4
    pair[0, 3:] = -torch.rand((3, H, W), generator=g) * 6e4
    pair[1, :3] = torch.randint(0, 40, (3, H, W), generator=g).float() * 2.0 ** -24
    flow = torch.zeros(B, 2, H, W)
    flow[0] = rnd(g, (2, H, W), 2.0)
    pair, flow = pair.to(dt).to(dev), flow.to(dt).to(dev)
    norm = fn2_capi.warp_diff_norm_16(pair, flow, True).float().cpu()
    assert bool(torch.isinf(norm[0]).any()) and bool(torch.isfinite(norm[0]).any())
    sub = (norm[1] > 0) & (norm[1] < 2.0 ** -14)
    assert int(sub.sum()) > H * W // 2                                          # the norms really are half subnormals
    check_all_levels(pair, flow, rnd(g, (B, 12, H, W)).to(dt).to(dev), rnd(g, (B, 1, H, W)).to(dt).to(dev), 20.0, True, "half range")


@pytest.mark.parametrize("dt", DTYPES, ids=["half", "bf16"])
@pytest.mark.parametrize("shape", [(2, 6, 32, 64), (2, 4, 10, 24)], ids=["tiled", "fallback"])
def test_inf_nan_and_zero_difference(dev, dt, shape):
    """inf and NaN in single pixels of the image and the flow (they spread exactly as in the float32 kernels), and a region where the
    first image equals the warped one: diff == 0, norm == 0, the gradient's norm + 1e-9 denominator."""
    B, C2, H, W = shape
    C = C2 // 2
    g = torch.Generator().manual_seed(7)
    pair, flow = rnd(g, shape, 0.5), rnd(g, (B, 2, H, W), 2.0)
    pair[0, C, 3, 5] = float("inf")
    pair[0, C + 1, 6, 9] = NAN
    pair[1, 0, 2, 2] = float("-inf")
    pair[1, 1, 4, 7] = NAN
    flow[0, 0, 7, 3] = NAN
    flow[0, 1, 1, 8] = float("inf")
    flow[1, 0, 5, 5] = float("-inf")
    flow[1, :, H // 2:, :] = 0.0
    pair[1, :C, H // 2:, :] = pair[1, C:, H // 2:, :]                           # zero flow, equal images: diff == 0
    pair, flow = pair.to(dt).to(dev), flow.to(dt).to(dev)
    assert float(fn2_capi.warp_diff_norm_16(pair, flow, True)[1, 0, H // 2 + 1:, :].float().abs().max()) == 0.0
    check_all_levels(pair, flow, rnd(g, (B, 3 * C + 3, H, W)).to(dt).to(dev), rnd(g, (B, 1, H, W)).to(dt).to(dev), 20.0, True, "specials")


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("dt", DTYPES, ids=["half", "bf16"])
def test_pair_gradient_takes_the_widened_path(dev, dt):
    """x.requires_grad: widened around the float32 node; grad_flow still bit-exact, grad_x 16-bit and within one 16-bit ulp of the
    float32 scatter's (atomics: order unspecified; the bound of test_bf16_resample2d)."""
    from networks.resample2d_package.resample2d import WarpDiffNorm, WarpDiffNormCat
    pair, flow, gcat, gn = make_case(dt, dev, RAGGED, "noise", 77)
    for mod, go in ((WarpDiffNormCat(20.0), gcat), (WarpDiffNorm(), gn)):
        x16, f16 = pair.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        x32, f32 = pair.float().requires_grad_(True), flow.float().requires_grad_(True)
        out, want = mod(x16, f16), mod(x32, f32)
        assert_bits(out, want, dt, "fwd")
        out.backward(go)
        want.backward(go.float())
        assert x16.grad.dtype == dt and f16.grad.dtype == dt
        assert_bits(f16.grad, f32.grad, dt, "grad_flow")
        gi = x32.grad
        assert bool(((x16.grad.float() - gi).abs() <= ULP1[dt] * gi.abs() + 1e-6 * float(gi.abs().max())).all())


@pytest.mark.parametrize("dt", DTYPES, ids=["half", "bf16"])
def test_mixed_dtypes_are_widened(dev, dt):
    """float32 pair with a 16-bit flow (autocast): widened, the output in the pair's type, the flow gradient in the flow's"""
    from networks.resample2d_package.resample2d import WarpDiffNorm, WarpDiffNormCat
    pair, flow, gcat, gn = make_case(dt, dev, RAGGED, "noise", 78)
    x = pair.float()
    for mod, go in ((WarpDiffNormCat(20.0), gcat), (WarpDiffNorm(), gn)):
        f16, f32 = flow.clone().requires_grad_(True), flow.float().requires_grad_(True)
        out, want = mod(x, f16), mod(x, f32)
        assert out.dtype == torch.float32 and torch.equal(out, want)
        out.backward(go.float())
        want.backward(go.float())
        assert_bits(f16.grad, f32.grad, dt, "grad_flow")


@pytest.mark.parametrize("dt", DTYPES, ids=["half", "bf16"])
def test_replay_from_a_hip_graph(dev, dt):
    """forward and backward of both modules captured into one (single-branch) graph; replays on new values equal the C ABI call"""
    from networks.resample2d_package.resample2d import WarpDiffNorm, WarpDiffNormCat
    pair, flow, gcat, gn = make_case(dt, dev, RAGGED, "noise", 79)
    flow.requires_grad_(True)
    wcat, wnorm = WarpDiffNormCat(20.0), WarpDiffNorm()

    def step():
        flow.grad = None
        o = wcat(pair, flow)
        o.backward(gcat)
        g1 = flow.grad
        flow.grad = None
        n = wnorm(pair, flow)
        n.backward(gn)
        return o.detach(), g1, n.detach(), flow.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    flow.grad = None
    with torch.cuda.graph(graph):
        captured = step()
    for seed in (80, 81):
        p2, f2, gc2, gn2 = make_case(dt, dev, RAGGED, "noise", seed)
        with torch.no_grad():
            pair.copy_(p2); flow.copy_(f2); gcat.copy_(gc2); gn.copy_(gn2)
        graph.replay()
        torch.cuda.synchronize()
        want = (fn2_capi.warp_diff_norm_cat_16(p2, f2, 20.0, True), fn2_capi.warp_diff_norm_cat_backward_16(p2, f2, gc2, 20.0, True),
                fn2_capi.warp_diff_norm_16(p2, f2, True), fn2_capi.warp_diff_norm_backward_16(p2, f2, gn2, True))
        for i, (a, b) in enumerate(zip(captured, want)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (seed, i)


@pytest.mark.parametrize("dt", DTYPES, ids=["half", "bf16"])
def test_two_threads_two_streams(dev, dt):
    """two threads, each on its own stream with its own inputs: every result is the one the same call gives alone"""
    from networks.resample2d_package.resample2d import WarpDiffNorm, WarpDiffNormCat
    args = [make_case(dt, dev, (4, 6, 192, 256), "noise", 90 + i) for i in range(2)]

    def run(pair, flow, gcat, gn):
        f = flow.clone().requires_grad_(True)
        o = WarpDiffNormCat(20.0)(pair, f)
        o.backward(gcat)
        f2 = flow.clone().requires_grad_(True)
        n = WarpDiffNorm()(pair, f2)
        n.backward(gn)
        return [o.detach(), f.grad, n.detach(), f2.grad]

    alone = [run(*a) for a in args]
    torch.cuda.synchronize()
    results, errors = [None, None], []
    start = threading.Barrier(2)

    def worker(i):
        try:
            st = torch.cuda.Stream(device=dev)
            st.wait_stream(torch.cuda.default_stream(dev))
            with torch.cuda.stream(st):
                start.wait()
                for _ in range(6):
                    r = run(*args[i])
                st.synchronize()
            results[i] = r
        except Exception as e:   # surfaced in the main thread
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    for i in range(2):
        for k, (a, b) in enumerate(zip(results[i], alone[i])):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (i, k)


@pytest.mark.parametrize("dt", DTYPES, ids=["half", "bf16"])
def test_no_fp32_temporaries(dev, dt):
    """A no-grad WarpDiffNormCat call at 8 x 6 x 384 x 512 allocates its output only (24 B/px): the peak above the memory held before the
    call stays below 2 x the output's bytes.  (Derived, not measured: the widened path holds the float32 pair, flow and output beside
    it, >= 104 B/px, more than 4 x; the factor 2 leaves room for the allocator's block rounding.)"""
    from networks.resample2d_package.resample2d import WarpDiffNormCat
    pair, flow, _, _ = make_case(dt, dev, BIG, "noise", 95)
    mod = WarpDiffNormCat(20.0)
    with torch.no_grad():
        out = mod(pair, flow)                 # warm-up
        out_bytes = out.numel() * out.element_size()
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = mod(pair, flow)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - before
    print("peak above the resident memory:", extra, "bytes; output:", out_bytes, "bytes")
    assert extra < 2 * out_bytes, (extra, out_bytes)


# ------------------------------------------------------------------------------------------------ harness
class _Widened(torch.nn.Module):
    """the composition the harness used before the native rows: row(x.float(), flow.float()).to(dtype)"""
    def __init__(self, row):
        super().__init__()
        self.row = row

    def forward(self, x, flow):
        return self.row(x.float(), flow.float()).to(x.dtype)


def test_harness_half_flownet2_same_bits(dev):
    """FlowNet2().half(), fixed seed, 1 x 2-frame 128 x 192.  One pass with forward hooks on the four warp sites: each site receives half
    tensors (the native rows are what runs) and its output has the bits of the widened composition on the very same inputs -- this
    part does not depend on the convolutions repeating from run to run.  The whole network is then run again with warp_cat / warp_err
    patched back to the widened composition: where two native passes repeat bit for bit (the convolution algorithms did not change
    between passes) the patched pass must give the same flow, bit for bit.  (On the MI355X the half convolutions did not repeat from pass
    to pass when this was written, so there the per-site comparison is what decides.)"""
    from harness.flownet2 import FlowNet2
    torch.manual_seed(3)
    net = FlowNet2().to(dev).eval().half()
    g = torch.Generator().manual_seed(4)
    inputs = (torch.rand(1, 3, 2, 128, 192, generator=g) * 255.0).to(dev).half()
    seen = []
    hooks = [m.register_forward_hook(lambda mod, args, out: seen.append((mod, args[0].detach().clone(), args[1].detach().clone(), out.detach().clone())))
             for m in (net.warp_cat, net.warp_err)]
    with torch.no_grad():
        flow_native = net(inputs)
        for h in hooks:
            h.remove()
        assert len(seen) == 4
        for mod, x, flow, out in seen:
            assert x.dtype == torch.float16 and flow.dtype == torch.float16 and out.dtype == torch.float16
            want = mod(x.float(), flow.float())
            assert_bits(out, want, torch.float16, type(mod).__name__)
        flow_again = net(inputs)
        net.warp_cat, net.warp_err = _Widened(net.warp_cat), _Widened(net.warp_err)
        flow_widened = net(inputs)
    assert flow_native.dtype == torch.float16 and torch.isfinite(flow_native).all()
    if torch.equal(flow_native, flow_again):
        assert torch.equal(flow_native.view(torch.int16), flow_widened.view(torch.int16))
    else:
        print("two native passes differ (convolution algorithms changed between passes): whole-network comparison not applicable")
