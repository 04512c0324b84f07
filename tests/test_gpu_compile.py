"""torch.compile over the HIP layers on the GPU: the ``fn2`` operators run the kernels the eager doors run.

1. ``torch.library.opcheck`` (default utilities) for every forward operator at the ragged shapes of tests/capi_graph_cases.py;
2. ``backend="aot_eager"`` against eager, per door and dtype, the same inputs: bit for bit -- the same kernels in the same order.  The
   three outputs summed by float atomics are compared under ``torch.use_deterministic_algorithms(True)`` where a fixed-point path
   exists (Resample2d's image gradient, the splat) and held to the header's float64 bound otherwise (CorrLookup's grad_fmap2,
   tests/corr_lookup_ref.py), never to the code under test;
3. both recipes compiled (forward-only twins, tests/compile_cases.py): bits against eager where no atomic lies upstream, the rule of
   tests/pipelines_ref.py against float64 for everything;
4. compiled mini-RAFT under float16 and bfloat16 autocast: the eager autocast run's bits;
5. errors and flags under compile: coords that require a gradient, a second backward, the deterministic flag;
6. Inductor, default and ``mode="reduce-overhead"`` (skipped without triton).
"""
import warnings

import numpy as np
import pytest
import torch
import torch._dynamo

import capi_graph_cases as G
import compile_cases as CC
import corr_lookup_ref as RL
import pipelines_ref as P

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _compile(fn, **kw):
    torch._dynamo.reset()
    return torch.compile(fn, fullgraph=True, **{"backend": "aot_eager", **kw})


def _bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    same = torch.equal(got.reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8)) if got.numel() else True
    assert same, f"{what}: {int((got != want).sum())} of {got.numel()} elements differ from the eager call"


class deterministic:
    def __init__(self, on=True, warn_only=False):
        self.on, self.warn_only = on, warn_only

    def __enter__(self):
        self.saved = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
        torch.use_deterministic_algorithms(self.on, warn_only=self.warn_only)

    def __exit__(self, *exc):
        torch.use_deterministic_algorithms(self.saved[0], warn_only=self.saved[1])


# ------------------------------------------------------------------ 1: opcheck
def _randn(shape, dev, seed, dtype=F32, grad=True, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev).requires_grad_(grad)


def _opcheck_rows(dev):
    import losses_fused  # noqa: F401
    import networks.census_package.census  # noqa: F401
    import networks.channelnorm_package.channelnorm  # noqa: F401
    import networks.correlation_package.corr_lookup  # noqa: F401
    import networks.correlation_package.correlation  # noqa: F401
    import networks.correlation_package.correlation1d  # noqa: F401
    import networks.resample2d_package.resample2d  # noqa: F401
    import networks.smoothness_package.smoothness  # noqa: F401
    import networks.splat_package.forward_warp  # noqa: F401
    import networks.upsample_package.convex_upsample  # noqa: F401
    ops = torch.ops.fn2
    rows = {}
    flownetc = next(r for r in G.CORR_ROWS if r[0] == "F16X2")
    dense = next(r for r in G.CORR_ROWS if r[0] == "DENSE")
    for tag, (_, _, shape, _, params) in (("flownetc", flownetc), ("dense", dense)):
        rows["correlation-" + tag] = (ops.correlation, (_randn(shape, dev, 1), _randn(shape, dev, 2)) + tuple(params) + (1,))
    shape, params = flownetc[2], flownetc[4]
    n_out, oH, oW = G.corr_out_shape(shape[2], shape[3], *params)
    rows["correlation_leakyrelu_cat"] = (ops.correlation_leakyrelu_cat, (_randn(shape, dev, 3), _randn(shape, dev, 4),
                                                                        _randn((shape[0], G.EXTRA, oH, oW), dev, 5)) + tuple(params) + (G.SLOPE,))
    shape1d, md = G.CORR1D
    rows["correlation1d"] = (ops.correlation1d, (_randn(shape1d, dev, 6), _randn(shape1d, dev, 7), md, md, 1, 1, 0))
    B, C, H, W = G.RESAMPLE
    rows["resample2d"] = (ops.resample2d, (_randn((B, C, H, W), dev, 8), _randn((B, 2, H, W), dev, 9, scale=2.0), 1, True))
    rows["channelnorm"] = (ops.channelnorm, (_randn(G.CHNORM, dev, 10), 2))
    B, C, H, W = G.PAIR_RAGGED
    pair, flow = (B, 2 * C, H, W), (B, 2, H, W)
    rows["warp_diff_norm_cat"] = (ops.warp_diff_norm_cat, (_randn(pair, dev, 11), _randn(flow, dev, 12, scale=2.0), G.DIV, True, True))
    rows["warp_diff_norm_cat-flow-only"] = (ops.warp_diff_norm_cat, (_randn(pair, dev, 11, grad=False), _randn(flow, dev, 12, scale=2.0), G.DIV, True, False))
    rows["warp_diff_norm"] = (ops.warp_diff_norm, (_randn(pair, dev, 13, grad=False), _randn(flow, dev, 14, scale=2.0), True))
    L = G.LOOKUP
    coords = G.lookup_coords(L["coords"], L["B"], *L["s1"], *L["s2"], L["r"], 3).to(dev)
    rows["corr_lookup"] = (ops.corr_lookup, (_randn((L["B"], L["C"]) + L["s1"], dev, 15), _randn((L["B"], L["C"]) + L["s2"], dev, 16), coords, L["r"],
                                             G.LOOKUP_SCALE))
    U = G.UPSAMPLE
    rows["convex_upsample"] = (ops.convex_upsample, (_randn((U["B"], U["C"], U["H"], U["W"]), dev, 17),
                                                     _randn((U["B"], 9 * U["f"] ** 2, U["H"], U["W"]), dev, 18), U["f"], float(U["f"])))
    B, C, H, W = G.SPLAT
    rows["forward_warp"] = (ops.forward_warp, (_randn((B, C, H, W), dev, 19), _randn((B, 2, H, W), dev, 20, scale=3.0)))
    rows["census"] = (ops.census, (torch.rand(G.CENSUS, device=dev).requires_grad_(True), torch.rand(G.CENSUS, device=dev).requires_grad_(True),
                                   3, 255.0, True))
    N, F, C, H, W = G.SMOOTH
    rows["smoothness"] = (ops.smoothness, (_randn((N, F, H, W), dev, 21), torch.rand((N, C, H, W), device=dev), 2, 0, 150.0, 0.001))
    target = _randn((2, 2, 128, 192), dev, 22, grad=False, scale=5.0)
    preds = [_randn((2, 2, 128 // (4 << i), 192 // (4 << i)), dev, 23 + i, scale=0.3) for i in range(5)]
    rows["multiscale_loss"] = (ops.multiscale_loss, (target, preds, 4, 0.05, [0.32 / 2 ** i for i in range(5)], 1))
    return rows


OPCHECK_IDS = ["correlation-flownetc", "correlation-dense", "correlation_leakyrelu_cat", "correlation1d", "resample2d", "channelnorm",
               "warp_diff_norm_cat", "warp_diff_norm_cat-flow-only", "warp_diff_norm", "corr_lookup", "convex_upsample", "forward_warp", "census",
               "smoothness", "multiscale_loss"]


@pytest.fixture(scope="module")
def opcheck_rows(dev):
    rows = _opcheck_rows(dev)
    assert sorted(rows) == sorted(OPCHECK_IDS)
    return rows


@pytest.mark.parametrize("which", OPCHECK_IDS)
def test_opcheck(opcheck_rows, which):
    op, args = opcheck_rows[which]
    torch.library.opcheck(op, args)


def test_every_forward_operator_is_opchecked(opcheck_rows):
    import fn2_ops
    forward = {n.split("::")[1] for n in fn2_ops.names() if not n.endswith("_backward")}
    assert forward == {w.split("-")[0] for w in OPCHECK_IDS}


# ------------------------------------------------------------------ 2: aot_eager against eager, per door
DET_DOORS = ("Resample2d", "WarpDiffNormCat-pair-grad", "WarpDiffNorm-pair-grad", "ForwardWarp", "softsplat", "range_map")   # a fixed-point path exists
LOOKUP_DOORS = ("CorrLookup", "CorrLookupFunction.apply", "AlternateCorrBlock")                                               # none: the float64 bound


def _run_door(fn, door, dtypes, dev):
    args = CC.make_inputs(door, dtypes, dev, seed=5)
    out = fn(*args)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(6)).to(out.dtype).to(dev)
    wanted = [a for a in args if a.requires_grad]
    return args, out.detach(), go, torch.autograd.grad(out, wanted, go)


def _lookup_grad2_bound(door, args, go):
    """(exact, bound) of grad_fmap2 in float64: the header's any-order bound for a single lookup; for the two-level block, whose
    fmap2 gradient also runs through the pooling, the rule of tests/pipelines_ref.py on the float64 and float32 compositions."""
    f1, f2, co = (a.detach().cpu() for a in args)
    if door.id == "AlternateCorrBlock":
        def grad(dtype):
            a, b = f1.to(dtype), f2.to(dtype).requires_grad_(True)
            out = RL.compose(a, b, co.to(dtype), 3, float(a.shape[1]) ** -0.5, num_levels=2)
            return torch.autograd.grad(out, b, go.cpu().to(dtype))[0]
        g64 = grad(torch.float64)
        return g64.numpy(), np.full(g64.shape, P.rule_bound(grad(torch.float32), g64))
    r, scale = (3, float(f1.shape[1]) ** -0.5) if door.id == "CorrLookup" else (2, 0.5)
    _, (e2, S2, n2) = RL.backward(f1.numpy(), f2.numpy(), co.numpy(), go.cpu().numpy(), r, scale)
    return e2, RL.delta_grad2(e2, S2, n2, scale)


@pytest.mark.parametrize("case", CC.door_cases(), ids=CC.case_id)
def test_aot_eager_is_eager(dev, case):
    door, dtypes = case
    fn = door.make()
    with deterministic(door.id.startswith(DET_DOORS)):
        args, out, go, grads = _run_door(fn, door, dtypes, dev)
        _, cout, _, cgrads = _run_door(_compile(fn), door, dtypes, dev)
    _bits(cout, out, door.id + " output")
    wanted = [i for i, a in enumerate(args) if a.requires_grad]
    for i, g, cg in zip(wanted, grads, cgrads):
        if door.id in LOOKUP_DOORS and i == 1:       # grad_fmap2: float atomics in arrival order, no fixed-point path
            exact, bound = _lookup_grad2_bound(door, args, go)
            for name, t in (("eager", g), ("compiled", cg)):
                err = np.abs(t.double().cpu().numpy() - exact)
                print(f"  {door.id} grad_fmap2 {name}: max error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
                assert (err <= bound).all(), f"{door.id}: {name} grad_fmap2 outside its float64 bound"
        else:
            _bits(cg, g, f"{door.id} gradient of argument {i}")


# ------------------------------------------------------------------ 3: the recipes
def _cast(inputs, dev, dtype=F32):
    return {k: torch.from_numpy(v).to(device=dev, dtype=dtype) for k, v in inputs.items()}


@pytest.fixture(scope="module")
def raft(dev):
    inp = P.raft_inputs()
    return dict(t=_cast(inp, dev), out32=P.run(P.mini_raft, inp, torch.float32, dev), out64=P.run(P.mini_raft, inp, torch.float64, dev))


@pytest.fixture(scope="module")
def unsup(dev):
    inp = P.unsup_inputs()
    P.check_unsup_inputs(inp)
    return dict(t=_cast(inp, dev), out32=P.run(P.unsup_loss, inp, torch.float32, dev), out64=P.run(P.unsup_loss, inp, torch.float64, dev))


# What of mini-RAFT is compared bit for bit: the flows, the loss and fmap1.grad.  Not compared that way: fmap2.grad and the feature
# network's gradients (downstream of CorrLookup's grad_fmap2, float atomics), and the other convolutions' parameter gradients, whose bits
# differ between the compiled and the eager run.  Measured under autocast (test_mini_raft_autocast_compiled prints it): the weight
# gradients differ between two EAGER runs as well, by as much (update.weight.grad under float16: 0.0156 either way -- MIOpen's
# weight-gradient kernels); the bias gradients repeat in eager and differ in the compiled run by an ulp or two of the 16-bit format
# (AOT autograd adds the three iterations' gradients in another order than the eager engine).
# In float32 all of them are held to float64 by the rule of tests/pipelines_ref.py; under autocast, to the eager autocast run (below).
RAFT_BITS = ("flow_up_0", "flow_up_1", "flow_up_2", "loss", "fmap1.grad")


def test_mini_raft_compiled(dev, raft):
    layers = P.hip_layers()
    eager = CC.run_mini_raft(CC.mini_raft_forward, layers, raft["t"])
    compiled = CC.run_mini_raft(_compile(CC.mini_raft_forward), layers, raft["t"])
    assert sorted(compiled) == sorted(raft["out64"])
    for k in RAFT_BITS:
        _bits(compiled[k], eager[k], "mini-RAFT " + k)
    assert P.rule_misses(compiled, raft["out32"], raft["out64"], "compiled mini-RAFT ") == []


def test_unsup_loss_compiled(dev, unsup):
    layers = P.hip_layers()
    with deterministic():       # im2.grad is Resample2d's image gradient, the range map a splat: their fixed-point paths
        eager = CC.run_unsup(CC.unsup_forward, layers, unsup["t"])
        compiled = CC.run_unsup(_compile(CC.unsup_forward), layers, unsup["t"])
    for k in compiled:
        _bits(compiled[k], eager[k], "unsupervised loss " + k)
    plain = CC.run_unsup(_compile(CC.unsup_forward), layers, unsup["t"])
    assert P.rule_misses(plain, unsup["out32"], unsup["out64"], "compiled unsupervised loss ") == []
    assert P.rule_misses(compiled, unsup["out32"], unsup["out64"], "compiled unsupervised loss, deterministic ") == []


# ------------------------------------------------------------------ 3b: the MultiScale criterion
@pytest.mark.parametrize("norm", ["L1", "L2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_multiscale_compiled_is_eager(dev, norm, dtype):
    """fn2::multiscale_loss is multiscale_loss_cuda.apply; its backward operator runs the pass again for the unit gradients: loss, metric
    and every gradient have the eager node's bits, a prediction that wants none gets none."""
    from losses_fused import MultiScale
    crit = MultiScale(norm=norm)
    target = _randn((2, 2, 128, 192), dev, 1, grad=False, scale=5.0)

    def run(fn):
        preds = [_randn((2, 2, 128 // (4 << i), 192 // (4 << i)), dev, 2 + i, dtype=dtype, grad=(i != 2), scale=0.3) for i in range(5)]
        loss, epe = fn(tuple(preds), target)
        (2.5 * loss).backward()
        return loss.detach(), epe.detach(), preds

    loss, epe, preds = run(crit)
    closs, cepe, cpreds = run(_compile(crit))
    _bits(closs, loss, "MultiScale loss")
    _bits(cepe, epe, "MultiScale EPE")
    assert preds[2].grad is None and cpreds[2].grad is None
    for i in (0, 1, 3, 4):
        assert bool((preds[i].grad != 0).any())
        _bits(cpreds[i].grad, preds[i].grad, f"MultiScale gradient of prediction {i}")


# ------------------------------------------------------------------ 4: autocast
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_mini_raft_autocast_compiled(dev, raft, dtype):
    layers = P.hip_layers()
    kw = dict(context=lambda: torch.autocast("cuda", dtype=dtype), upsample_input=lambda f: f.float())
    eager = CC.run_mini_raft(CC.mini_raft_forward, layers, raft["t"], **kw)
    compiled = CC.run_mini_raft(_compile(CC.mini_raft_forward), layers, raft["t"], **kw)
    again = CC.run_mini_raft(CC.mini_raft_forward, layers, raft["t"], **kw)
    for k in RAFT_BITS:
        _bits(compiled[k], eager[k], f"mini-RAFT under {dtype} autocast, {k}")
    # The other gradients (their bits differ from the eager run's, as in float32), against the eager autocast run: inside
    #     max(8 max |eager - eager again|, 16 half-ulps of the autocast dtype at the tensor's scale)
    # -- the rule of tests/pipelines_ref.py with the eager run's own spread as the yardstick.  The floor is in the autocast dtype because that
    # is where these sums are rounded: a parameter is cast once per autocast region, so the three iterations' gradients meet in 16 bits,
    # and the order in which they are added (the eager engine's, AOT autograd's) moves the sum by ulps of that format.
    half_ulp = 2.0 ** -(11 if dtype == torch.float16 else 8)
    for k in sorted(set(compiled) - set(RAFT_BITS)):
        assert compiled[k].dtype == eager[k].dtype and compiled[k].shape == eager[k].shape, k
        e, a, c = (t[k].double() for t in (eager, again, compiled))
        own, err, scale = float((e - a).abs().max()), float((c - e).abs().max()), float(e.abs().max())
        bound = max(8 * own, 16 * half_ulp * scale)
        print(f"  {dtype} autocast {k}: compiled - eager {err:.3g}, eager - eager again {own:.3g}, bound {bound:.3g} (scale {scale:.3g})")
        assert err <= bound, f"mini-RAFT under {dtype} autocast, {k}: {err:.3g} from the eager run, bound {bound:.3g}"


# ------------------------------------------------------------------ 5: errors and flags under compile
def _lookup_args(dev, coords_grad=False):
    f1, f2 = _randn((2, 8, 9, 11), dev, 1), _randn((2, 8, 5, 6), dev, 2)
    return f1, f2, _randn((2, 2, 9, 11), dev, 3, grad=coords_grad, scale=2.0)


def test_coords_requiring_grad_raise_under_compile(dev):
    from networks.correlation_package import CorrLookup
    with pytest.raises(Exception, match="coords requires grad"):
        _compile(CorrLookup(3))(*_lookup_args(dev, coords_grad=True))


def test_second_backward_raises_under_compile(dev):
    from networks.correlation_package.correlation import Correlation
    a, b = _randn((2, 8, 9, 11), dev, 1), _randn((2, 8, 9, 11), dev, 2)
    out = _compile(Correlation(3, 1, 3, 1, 2, 1))(a, b)
    out.sum().backward()
    with pytest.raises(RuntimeError, match="second time|already been freed"):
        out.sum().backward()


def test_deterministic_flag_repeats_the_compiled_unsup_recipe(dev, unsup):
    layers, fn = P.hip_layers(), _compile(CC.unsup_forward)
    with deterministic():
        first = CC.run_unsup(fn, layers, unsup["t"])
        second = CC.run_unsup(fn, layers, unsup["t"])
    for k in first:
        _bits(second[k], first[k], "deterministic compiled recipe, second run, " + k)


def test_deterministic_flag_refuses_compiled_lookup_backward(dev):
    from networks.correlation_package import CorrLookup
    fn = _compile(CorrLookup(3))
    with deterministic():
        out = fn(*_lookup_args(dev))
        with pytest.raises(RuntimeError, match="corr_lookup_cuda.backward"):
            out.sum().backward()
    with deterministic(warn_only=True):
        out = fn(*_lookup_args(dev))
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out.sum().backward()
        assert any("corr_lookup_cuda.backward" in str(w.message) for w in caught), [str(w.message) for w in caught]


# ------------------------------------------------------------------ 6: Inductor
def _corr_and_pointwise(a, b):
    out = torch.ops.fn2.correlation(a, b, 3, 1, 3, 1, 2, 1)       # the operator's inputs are graph inputs, its raw result an output
    return out, torch.tanh(out) * 2.0 + a.mean()


def test_inductor_default(dev):
    pytest.importorskip("triton")
    import networks.correlation_package.correlation  # noqa: F401
    a, b = _randn((2, 8, 9, 11), dev, 1, grad=False), _randn((2, 8, 9, 11), dev, 2, grad=False)
    want, want_pointwise = _corr_and_pointwise(a, b)
    torch._dynamo.reset()
    got, got_pointwise = torch.compile(_corr_and_pointwise, fullgraph=True)(a, b)
    _bits(got, want, "correlation inside an Inductor graph")
    torch.testing.assert_close(got_pointwise, want_pointwise)


def test_inductor_reduce_overhead_replays(dev):
    """Four calls on fresh values, three of them replays of the captured graphs: the operator's bits, and the unsupervised recipe's
    loss and gradients by the rule of tests/pipelines_ref.py against float64 each time (Inductor fuses the pointwise parts, so the
    recipe's bits are not eager's).  ForwardWarp's clear is a kernel, so it replays."""
    pytest.importorskip("triton")
    import networks.correlation_package.correlation  # noqa: F401
    from torch._dynamo.utils import counters
    layers = P.hip_layers()
    torch._dynamo.reset()
    counters.clear()
    fn = torch.compile(CC.unsup_forward, fullgraph=True, mode="reduce-overhead")
    for seed in range(4):
        inp = P.unsup_inputs(seed=seed)
        P.check_unsup_inputs(inp)
        got = {k: v.clone() for k, v in CC.run_unsup(fn, layers, _cast(inp, dev)).items()}
        out32, out64 = P.run(P.unsup_loss, inp, torch.float32, dev), P.run(P.unsup_loss, inp, torch.float64, dev)
        assert P.rule_misses(got, out32, out64, f"reduce-overhead call {seed} ") == []
    torch._dynamo.reset()
    corr = torch.compile(_corr_and_pointwise, fullgraph=True, mode="reduce-overhead")
    for seed in range(4):
        a, b = _randn((2, 8, 9, 11), dev, 10 + seed, grad=False), _randn((2, 8, 9, 11), dev, 20 + seed, grad=False)
        _bits(corr(a, b)[0].clone(), _corr_and_pointwise(a, b)[0], f"correlation, reduce-overhead call {seed}")
    # Inductor turns CUDA graphs off for reasons it only logs; then nothing above was a replay
    assert counters["inductor"]["cudagraph_skips"] == 0, dict(counters["inductor"])
    from torch._inductor import cudagraph_trees
    assert cudagraph_trees.get_container(dev.index).tree_manager is not None, "no CUDA graph tree was built"
