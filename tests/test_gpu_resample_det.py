"""The deterministic image gradient of Resample2d and WarpDiffNormCat on the GPU: under torch.use_deterministic_algorithms(True) the
backward passes sum grad_input1 in fixed point (fn2_*_backward_det), and the result must equal the numpy restatement of the contract
(tests/resample_det_ref.py) bit for bit, on every kernel path; grad_flow must equal the default path's."""
import contextlib
import threading

import numpy as np
import pytest
import torch

import resample_det_ref as R

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def deterministic(warn_only=False):
    prev, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=warn_only)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)


DEV = torch.device("cuda:0")


def bits(t):
    a = t.detach().float().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bits(got, want, what=""):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        n = int(np.count_nonzero(g != w))
        raise AssertionError(f"{what}: {n} of {g.size} elements differ bitwise")


def run_backward(img, flow, gout, k=1, g1_init=None):
    """resample2d_cuda.backward on device tensors; grad_flow prefilled with NaN so that an unwritten element shows."""
    import resample2d_cuda
    g1 = torch.zeros_like(img) if g1_init is None else g1_init.clone()
    if not img.is_contiguous():
        g1 = g1.contiguous()
    g2 = torch.full_like(flow, float("nan"))
    assert resample2d_cuda.backward(img, flow, gout, g1, g2, k, True) == 1
    torch.cuda.synchronize()
    return g1, g2


def case(B, C, Hi, Wi, H, W, flow_kind="bench", seed=0):
    rng = np.random.default_rng(seed)
    img = torch.from_numpy(rng.standard_normal((B, C, Hi, Wi)).astype(np.float32))
    if flow_kind == "bench":
        flow = R.bench_flow(B, H, W, seed)
    elif flow_kind == "translate":
        flow = R.translated_flow(B, H, W, seed)
    else:
        flow = R.sink_flow(B, H, W, seed)
    gout = rng.standard_normal((B, C, H, W)).astype(np.float32)
    return img.to(DEV), torch.from_numpy(flow).to(DEV), torch.from_numpy(gout).to(DEV)


def check_against_helper(img, flow, gout, k=1, g1_init=None):
    with deterministic():
        g1, g2 = run_backward(img, flow, gout, k, g1_init)
    init = None if g1_init is None else g1_init.cpu().numpy()
    want = R.resample_bwd_det(tuple(img.shape), flow.cpu().numpy(), gout.cpu().numpy(), k, grad_init=init)
    assert_bits(g1, want, "grad_input1 vs the helper")
    _, g2_default = run_backward(img, flow, gout, k)
    assert not torch.isnan(g2).any(), "grad_flow left at its NaN prefill"
    assert_bits(g2, g2_default, "grad_flow vs the default path")
    return g1, g2


@pytest.mark.parametrize("flow_kind", ["bench", "translate", "sink"])
def test_flownet2_shape_bitwise(flow_kind):
    img, flow, gout = case(8, 3, 384, 512, 384, 512, flow_kind, seed=1)
    check_against_helper(img, flow, gout)


@pytest.mark.parametrize("shape", [
    (2, 1, 64, 96, 64, 96, 1), (2, 2, 64, 96, 64, 96, 1), (2, 5, 48, 64, 48, 64, 1), (1, 64, 40, 72, 40, 72, 1),   # tiled, C != 3
    (2, 3, 64, 96, 64, 96, 2), (2, 5, 20, 36, 20, 36, 3),                                                        # kernel_size > 1
    (3, 3, 12, 24, 12, 24, 1),                                                                                   # smaller than a tile
    (2, 3, 40, 70, 40, 70, 1),                                                                                   # W % 4 != 0
    (2, 3, 50, 60, 40, 64, 1), (1, 2, 30, 44, 36, 48, 2),                                                        # Hi x Wi != H x W
])
def test_paths_bitwise(shape):
    B, C, Hi, Wi, H, W, k = shape
    img, flow, gout = case(B, C, Hi, Wi, H, W, "sink" if C % 2 else "bench", seed=B * 100 + C)
    check_against_helper(img, flow, gout, k)


def test_strided_input1():
    """a channel slice of a wider tensor: the image's strides are honoured, grad_input1 is contiguous."""
    img6, flow, gout = case(2, 6, 64, 96, 64, 96, "bench", seed=7)
    img = img6[:, 3:]
    assert not img.is_contiguous()
    check_against_helper(img, flow, gout[:, :3].contiguous())


def test_accumulates_into_prefilled_grad():
    img, flow, gout = case(2, 3, 64, 128, 64, 128, "bench", seed=8)
    init = torch.randn(img.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    check_against_helper(img, flow, gout, g1_init=init)


def test_nonfinite_plane_is_serial_and_isolated(oracle):
    img, flow, gout = case(2, 3, 20, 40, 20, 40, "bench", seed=9)
    gout[1, 2, 5, 7] = float("inf")
    gout[0, 0, 3, 3] = float("nan")
    with deterministic():
        g1, g2 = run_backward(img, flow, gout)
    ref, _ = oracle.resample_bwd(img.cpu().numpy(), flow.cpu().numpy(), gout.cpu().numpy())
    want = R.resample_bwd_det(tuple(img.shape), flow.cpu().numpy(), gout.cpu().numpy())
    for b, c in [(1, 2), (0, 0)]:
        assert_bits(g1[b, c], ref[b, c], f"non-finite plane {(b, c)} vs the serial oracle")
    for b, c in [(0, 1), (0, 2), (1, 0), (1, 1)]:
        assert_bits(g1[b, c], want[b, c], f"finite plane {(b, c)} vs the helper")


def test_batch_item_independent_of_batch():
    img, flow, gout = case(8, 3, 96, 128, 96, 128, "sink", seed=10)
    with deterministic():
        full, _ = run_backward(img, flow, gout)
        for b in (0, 5):
            one, _ = run_backward(img[b:b + 1].contiguous(), flow[b:b + 1].contiguous(), gout[b:b + 1].contiguous())
            assert_bits(one[0], full[b], f"item {b} alone vs in B = 8")


def test_two_threads_two_streams_bitwise():
    args = [case(4, 3, 192, 256, 192, 256, kind, seed=20 + i) for i, kind in enumerate(["bench", "sink"])]
    with deterministic():
        alone = [run_backward(*a) for a in args]
        results, errors = [None, None], []
        start = threading.Barrier(2)

        def worker(i):
            try:
                st = torch.cuda.Stream(device=DEV)
                st.wait_stream(torch.cuda.default_stream(DEV))
                with torch.cuda.stream(st):
                    import resample2d_cuda
                    start.wait()
                    for _ in range(4):
                        img, flow, gout = args[i]
                        g1, g2 = torch.zeros_like(img), torch.empty_like(flow)
                        resample2d_cuda.backward(img, flow, gout, g1, g2, 1, True)
                    st.synchronize()
                results[i] = (g1, g2)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        # the deterministic flag is process-global: the worker threads see it
        ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    assert not errors, errors
    for i in range(2):
        assert_bits(results[i][0], alone[i][0], f"thread {i} grad_input1")
        assert_bits(results[i][1], alone[i][1], f"thread {i} grad_flow")


def test_modules_take_the_deterministic_path():
    import resample2d_cuda
    from networks.resample2d_package.resample2d import Resample2d, Resample2dFunction
    img, flow, gout = case(2, 3, 64, 96, 64, 96, "sink", seed=30)
    want = R.resample_bwd_det(tuple(img.shape), flow.cpu().numpy(), gout.cpu().numpy())
    _, gflow_default = run_backward(img, flow, gout)
    with deterministic(warn_only=True):
        g = resample2d_cuda.backward_alloc(img, flow, gout, 1, True)
        assert_bits(g[0], want, "backward_alloc")
        assert_bits(g[1], gflow_default, "backward_alloc grad_flow")
        for name, fn in [("C++ node", lambda a, f: Resample2d()(a, f)),
                         ("Python Function", lambda a, f: super(Resample2dFunction, Resample2dFunction).apply(a, f, 1, True))]:
            a, f = img.clone().requires_grad_(True), flow.clone().requires_grad_(True)
            fn(a, f).backward(gout)
            assert_bits(a.grad, want, name)
            assert_bits(f.grad, gflow_default, name + " grad_flow")


def test_bf16_rounds_the_fp32_result_once():
    import resample2d_cuda
    img, flow, gout = case(2, 3, 64, 96, 64, 96, "bench", seed=31)
    ib, fb, gb = img.bfloat16(), flow.bfloat16(), gout.bfloat16()
    want = R.resample_bwd_det(tuple(img.shape), fb.float().cpu().numpy(), gb.float().cpu().numpy())
    with deterministic():
        g1, g2 = torch.zeros_like(ib), torch.empty_like(fb)
        assert resample2d_cuda.backward(ib, fb, gb, g1, g2, 1, True) == 1
    assert g1.dtype == torch.bfloat16
    assert_bits(g1, torch.from_numpy(want).bfloat16(), "bf16 grad_input1")


@pytest.mark.parametrize("shape", [(2, 3, 64, 128), (2, 3, 30, 44), (1, 2, 40, 64)])   # tiled C = 3, untiled, C != 3
def test_warp_diff_norm_cat_pair_gradient(shape):
    from networks.resample2d_package.resample2d import WarpDiffNormCat
    B, C, H, W = shape
    rng = np.random.default_rng(40 + C)
    x = torch.from_numpy(rng.standard_normal((B, 2 * C, H, W)).astype(np.float32)).to(DEV)
    flow = torch.from_numpy(R.sink_flow(B, H, W, seed=C)).to(DEV)
    gcat = torch.from_numpy(rng.standard_normal((B, 3 * C + 3, H, W)).astype(np.float32)).to(DEV)
    mod = WarpDiffNormCat(div_flow=20.0)

    def grads():
        xa, fa = x.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        out = mod(xa, fa)
        out.backward(gcat)
        torch.cuda.synchronize()
        return out.detach(), xa.grad, fa.grad

    out, gx_default, gf_default = grads()
    with deterministic():
        out_d, gx, gf = grads()
    assert_bits(out_d, out, "forward")
    want = R.warp_diff_norm_cat_grad_second(x.cpu().numpy(), flow.cpu().numpy(), out.cpu().numpy(), gcat.cpu().numpy())
    assert_bits(gx[:, C:], want, "second image's gradient vs the helper")
    assert_bits(gx[:, :C], gx_default[:, :C], "first image's gradient vs the default path")
    assert_bits(gf, gf_default, "flow gradient vs the default path")


def test_flownet2_layers_repeat_bitwise():
    """Correlation + Resample2d + ChannelNorm forward and backward at FlowNet2 shapes, twice under the flag: the same bits."""
    from networks.channelnorm_package.channelnorm import ChannelNorm
    from networks.correlation_package.correlation import Correlation
    from networks.resample2d_package.resample2d import Resample2d
    g = torch.Generator().manual_seed(50)
    f1, f2 = torch.randn(4, 256, 48, 64, generator=g).to(DEV), torch.randn(4, 256, 48, 64, generator=g).to(DEV)
    img = torch.randn(4, 3, 384, 512, generator=g).to(DEV)
    flow = (torch.randn(4, 2, 384, 512, generator=g) * 4).to(DEV)
    corr, warp, norm = Correlation(20, 1, 20, 1, 2, 1), Resample2d(), ChannelNorm()

    def once():
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        im, fl = img.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        c = corr(a, b)
        n = norm(warp(im, fl))
        (c.square().mean() + n.sum()).backward()
        torch.cuda.synchronize()
        return [c.detach(), n.detach(), a.grad, b.grad, im.grad, fl.grad]

    with deterministic():
        r1, r2 = once(), once()
    for i, (x, y) in enumerate(zip(r1, r2)):
        assert_bits(x, y, f"result {i}")


def test_backward_replays_from_a_hip_graph():
    """The deterministic backward sums in an int64 workspace that the entry point clears on the stream; captured into a hipGraph
    that clear has to run on EVERY replay (a workspace left as it was adds the last replay's sums).  Resample2d's forward and
    backward are captured once under the flag and replayed on three sets of values in the captured buffers: the bits of the
    eager deterministic call."""
    from networks.resample2d_package.resample2d import Resample2d
    img, flow, gout = case(2, 3, 40, 72, 40, 72, "bench", seed=20)
    img.requires_grad_(True)
    flow.requires_grad_(True)
    layer = Resample2d()

    def step():
        return torch.autograd.grad(layer(img, flow), (img, flow), gout)

    with deterministic():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g1, g2 = step()
        for kind, seed in (("translate", 21), ("sink", 22), ("bench", 23)):
            fresh = case(2, 3, 40, 72, 40, 72, kind, seed=seed)
            with torch.no_grad():
                for dst, src in zip((img, flow, gout), fresh):
                    dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            e1, e2 = run_backward(*fresh)
            assert_bits(g1, e1, f"grad_input1 replayed, {kind}")
            assert_bits(g2, e2, f"grad_flow replayed, {kind}")
