"""torch.compile over the HIP layers without a GPU: every public door traces under ``backend="aot_eager", fullgraph=True`` on
``device="meta"`` tensors, forward and backward, through the ``fn2`` operators (flownet2-pytorch_amd/fn2_ops.py).

1. every door of tests/compile_cases.py, in every dtype the eager door accepts: the output and the gradients have the documented
   shape and dtype;
2. the two recipes of INTEGRATION.md (forward-only twins of tests/pipelines_ref.py) trace end to end, with zero graph breaks;
3. harness.FlowNet2C traces at its smallest input, train() and eval(), fused rows and the three separate ops;
4. the fake shapes of Correlation and Correlation1d equal the C functions' over a sweep of their parameters, refusals included;
5. what shapes and parameters alone decide is refused at trace time, and so are coords / an image that require a gradient;
6. importing one layer registers that layer's operators and loads that layer's extension, no other;
7. under ``dynamic=True`` a second call at another spatial size does not compile again.

8. the MultiScale criterion traces, alone and on harness.FlowNet2C's outputs;
9. ``make_fx`` and ``torch.export`` see the operators: called directly, and through a Module under ``strict=True`` (Dynamo).

On the parent commit these fail with Dynamo's "unsupported" error at the first pybind builtin, or for want of the operators; the C side
of 4 does not depend on the change.
"""
import itertools
import subprocess
import sys
import types

import pytest
import torch
import torch._dynamo
from torch._dynamo.testing import CompileCounterWithBackend

import compile_cases as CC
import fn2_capi
import pipelines_ref as P

META = torch.device("meta")


def _compile(fn, **kw):
    torch._dynamo.reset()
    return torch.compile(fn, backend="aot_eager", fullgraph=True, **kw)


def _meta_inputs(door, dtypes, shapes=None):
    return [torch.empty(shape if shapes is None else shapes[i], dtype=dt, device=META, requires_grad=need)
            for i, ((shape, _, need), dt) in enumerate(zip(door.inputs, dtypes))]


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", CC.door_cases(), ids=CC.case_id)
def test_door_traces_forward_and_backward(case):
    door, dtypes = case
    args = _meta_inputs(door, dtypes)
    out = _compile(door.make())(*args)
    wanted = [a for a in args if a.requires_grad]
    assert out.device.type == "meta" and out.requires_grad
    assert out.dtype == args[0].dtype, (out.dtype, args[0].dtype)       # every door answers in its first argument's dtype
    grads = torch.autograd.grad(out.sum(), wanted)
    for g, a in zip(grads, wanted):
        assert g.shape == a.shape and g.dtype == a.dtype, (door.id, g.shape, g.dtype, a.shape, a.dtype)


DOCUMENTED_SHAPES = {       # what the eager doors document for the inputs of compile_cases.DOORS
    "Correlation": (2, 9, 9, 11), "CorrelationLeakyReLUCat": (2, 5 + 9, 9, 11), "Correlation1d": (2, 9, 9, 11),
    "Correlation1dFunction.apply": (2, 3, 9, 7), "Resample2d": (2, 3, 9, 11), "WarpDiffNormCat": (2, 12, 9, 11), "WarpDiffNorm": (2, 1, 9, 11),
    "WarpDiffNorm-pair-grad": (2, 1, 9, 11), "ChannelNorm": (2, 1, 9, 11), "CorrLookup": (2, 49, 9, 11), "CorrLookupFunction.apply": (2, 25, 9, 11),
    "AlternateCorrBlock": (2, 98, 9, 11), "ConvexUpsample": (2, 2, 36, 44), "ConvexUpsampleFunction.apply": (2, 2, 18, 22),
    "upsample_flow": (2, 2, 72, 88), "ForwardWarp": (2, 3, 9, 11), "softsplat-avg": (2, 3, 9, 11), "softsplat-soft": (2, 3, 9, 11),
    "range_map": (2, 1, 9, 11), "census_distance": (2, 1, 9, 11), "TernaryCensus": (2, 1, 9, 11), "CensusLoss": (), "smoothness_map": (2, 2, 9, 11),
    "EdgeAwareSmoothness": (2, 2, 9, 11), "SmoothnessLoss": (),
    "CorrelationFunction.apply": (2, 25, 5, 7), "Resample2dFunction.apply": (2, 3, 9, 11), "WarpDiffNormCat-pair-grad": (2, 12, 9, 11),
    "WarpDiffNormCatFunction.apply": (2, 12, 9, 11), "WarpDiffNormFunction.apply": (2, 1, 9, 11), "ChannelNormFunction.apply": (2, 1, 9, 11),
    "ForwardWarpFunction.apply": (2, 3, 9, 11), "softsplat-sum": (2, 3, 9, 11), "softsplat-linear": (2, 3, 9, 11),
    "CensusFunction.apply": (2, 1, 9, 11), "SmoothnessFunction.apply": (2, 2, 9, 11),
}
assert sorted(DOCUMENTED_SHAPES) == sorted(CC.DOOR_IDS)


@pytest.mark.parametrize("door_id", sorted(DOCUMENTED_SHAPES))
def test_door_output_shape(door_id):
    door = CC.DOORS[CC.DOOR_IDS.index(door_id)]
    out = _compile(door.make())(*_meta_inputs(door, [s[1] for s in door.inputs]))
    assert tuple(out.shape) == DOCUMENTED_SHAPES[door_id]
    assert out.is_contiguous()


# ------------------------------------------------------------------ 2
def _meta(d, dtype=torch.float32):
    return {k: torch.empty(v.shape, dtype=dtype, device=META) for k, v in d.items()}


@pytest.fixture(scope="module")
def raft_meta():
    return _meta(P.raft_inputs())


@pytest.fixture(scope="module")
def unsup_meta():
    return _meta(P.unsup_inputs())


def test_mini_raft_traces(raft_meta):
    out = CC.run_mini_raft(_compile(CC.mini_raft_forward), P.hip_layers(), raft_meta)   # (the feature convolutions stay outside)
    N, H, W = P.RAFT_SHAPE
    assert all(out["flow_up_%d" % i].shape == (N, 2, H, W) for i in range(P.RAFT_ITERS)) and out["loss"].shape == ()
    assert out["fmap1.grad"].shape == out["fmap2.grad"].shape == (N, P.RAFT_CHANNELS, H // 8, W // 8)
    assert all(out[k + ".grad"].shape == raft_meta[k].shape and out[k + ".grad"].dtype == torch.float32 for k in P.RAFT_PARAMS)


def test_unsup_loss_traces(unsup_meta):
    out = CC.run_unsup(_compile(CC.unsup_forward), P.hip_layers(), unsup_meta)
    assert out["loss"].shape == out["photometric"].shape == out["smooth"].shape == ()
    assert out["noc"].shape == (P.UNSUP_SHAPE[0], 1) + P.UNSUP_SHAPE[1:]
    assert all(out[k + ".grad"].shape == unsup_meta[k].shape for k in ("im1", "im2", "flow12"))


def test_recipes_have_no_graph_breaks(raft_meta, unsup_meta):
    layers = P.hip_layers()
    torch._dynamo.reset()
    params = {k: raft_meta[k].detach().clone().requires_grad_(True) for k in P.RAFT_PARAMS}
    fmap = torch.empty((P.RAFT_SHAPE[0], P.RAFT_CHANNELS, P.RAFT_SHAPE[1] // 8, P.RAFT_SHAPE[2] // 8), device=META, requires_grad=True)
    rep = torch._dynamo.explain(CC.mini_raft_forward)(layers, raft_meta, params, fmap, fmap.clone(), None)
    assert rep.graph_break_count == 0 and rep.graph_count == 1, rep.break_reasons
    torch._dynamo.reset()
    im1, im2, flow12 = (unsup_meta[k].detach().clone().requires_grad_(True) for k in ("im1", "im2", "flow12"))
    rep = torch._dynamo.explain(CC.unsup_forward)(layers, im1, im2, flow12, unsup_meta["flow21"])
    assert rep.graph_break_count == 0 and rep.graph_count == 1, rep.break_reasons
    assert rep.op_count > 0


# ------------------------------------------------------------------ 3
@pytest.fixture(scope="module")
def flownet2c():
    from harness.flownet2c import FlowNet2C
    with torch.device("meta"):
        return {fused: FlowNet2C(fused_inference=fused, fused_training=fused) for fused in (True, False)}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_flownet2c_traces_in_training(flownet2c, fused):
    model = flownet2c[fused].train()
    frames = torch.empty(1, 3, 2, 64, 64, device=META)        # 64: six stride-2 convolutions down to 1 x 1
    flows = _compile(model)(frames)
    assert [tuple(f.shape) for f in flows] == [(1, 2, 64 >> k, 64 >> k) for k in (2, 3, 4, 5, 6)]
    grads = torch.autograd.grad(sum(f.sum() for f in flows), list(model.parameters()))
    assert all(g.shape == p.shape for g, p in zip(grads, model.parameters()))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_flownet2c_traces_in_eval(flownet2c, fused):
    model = flownet2c[fused].eval()
    with torch.no_grad():
        flow = _compile(model)(torch.empty(1, 3, 2, 64, 64, device=META))
    assert tuple(flow.shape) == (1, 2, 64, 64)


# ------------------------------------------------------------------ 4
def _c_or_none(fn, *a):
    try:
        return fn(*a)
    except RuntimeError:
        return None


def test_correlation_fake_shape_is_the_c_function():
    from networks.correlation_package.correlation import correlation_output_shape
    n = 0
    for H, W, pad, k, md, s1, s2 in itertools.product((1, 5, 8), (1, 6, 23), (0, 3, 20), (0, 1, 3, 4), (0, 3, 20), (0, 1, 2, 3), (0, 1, 2, 3)):
        want = _c_or_none(fn2_capi.correlation_output_shape, H, W, pad, k, md, s1, s2)
        got = _c_or_none(correlation_output_shape, H, W, pad, k, md, s1, s2)
        assert got == want, ((H, W, pad, k, md, s1, s2), got, want)
        n += want is not None
    assert n > 200
    assert _c_or_none(correlation_output_shape, 5, 6, -1, 1, 0, 1, 1) is None and _c_or_none(fn2_capi.correlation_output_shape, 5, 6, -1, 1, 0, 1, 1) is None
    # and the operator's fake answers with it
    a = torch.empty(2, 4, 8, 23, device=META)
    assert tuple(torch.ops.fn2.correlation(a, a, 3, 3, 4, 2, 2, 1).shape) == (2,) + fn2_capi.correlation_output_shape(8, 23, 3, 3, 4, 2, 2)


def test_correlation1d_fake_shape_is_the_c_function():
    from networks.correlation_package.correlation1d import correlation1d_output_shape
    n = 0
    for H, W, pad, md, s1, s2, sd in itertools.product((1, 5, 8), (1, 6, 23), (0, 3, 20), (0, 3, 4, 20), (0, 1, 2, 3), (0, 1, 2, 3), (-2, -1, 0, 1, 2)):
        want = _c_or_none(fn2_capi.correlation1d_output_shape, H, W, pad, md, s1, s2, sd)
        got = _c_or_none(correlation1d_output_shape, H, W, pad, md, s1, s2, sd)
        assert got == want, ((H, W, pad, md, s1, s2, sd), got, want)
        n += want is not None
    assert n > 200
    a = torch.empty(2, 4, 8, 23, device=META)
    assert tuple(torch.ops.fn2.correlation1d(a, a, 3, 4, 2, 1, -1).shape) == (2,) + fn2_capi.correlation1d_output_shape(8, 23, 3, 4, 2, 1, -1)


# ------------------------------------------------------------------ 5
def _t(*shape, dtype=torch.float32, grad=False):
    return torch.empty(*shape, dtype=dtype, device=META, requires_grad=grad)


def _refusals():
    from networks.census_package import TernaryCensus
    from networks.channelnorm_package.channelnorm import ChannelNorm
    from networks.correlation_package import CorrLookup, Correlation1d
    from networks.correlation_package.correlation import Correlation, CorrelationLeakyReLUCat
    from networks.resample2d_package.resample2d import Resample2d, WarpDiffNormCat
    from networks.smoothness_package import SmoothnessLoss
    from networks.splat_package import ForwardWarp
    from networks.upsample_package import ConvexUpsample
    pair = _t(2, 8, 9, 11)
    return [
        ("corr rank", Correlation(3, 1, 3, 1, 2, 1), (_t(8, 9, 11), _t(8, 9, 11)), "4-D"),
        ("corr shapes", Correlation(3, 1, 3, 1, 2, 1), (pair, _t(2, 8, 9, 12)), "same shape"),
        ("corr empty output", Correlation(0, 1, 20, 1, 2, 1), (pair, pair), "empty"),
        ("corr stride", Correlation(3, 1, 3, 0, 2, 1), (pair, pair), "invalid argument"),
        ("fused redir", CorrelationLeakyReLUCat(3, 1, 3, 1, 2, 0.1), (pair, pair, _t(2, 5, 9, 12)), "cannot hold"),
        ("corr1d direction", Correlation1d(4, 4, 1, 1, 2), (pair, pair), "invalid argument"),
        ("corr1d empty output", Correlation1d(0, 6, 1, 1, 0), (pair, pair), "empty"),
        ("lookup radius", CorrLookup(9), (pair, pair, _t(2, 2, 9, 11)), "radius 9 outside"),
        ("lookup channels", CorrLookup(3), (pair, _t(2, 7, 9, 11), _t(2, 2, 9, 11)), "batch and channel counts"),
        ("lookup half", CorrLookup(3), (pair.half(), pair.half(), _t(2, 2, 9, 11).half()), "float32 tensors expected"),
        ("lookup coords grad", CorrLookup(3), (pair, pair, _t(2, 2, 9, 11, grad=True)), "coords requires grad"),
        ("resample flow channels", Resample2d(), (_t(2, 3, 9, 11), _t(2, 3, 9, 11)), "2 channels"),
        ("resample half", Resample2d(), (_t(2, 3, 9, 11).half(), _t(2, 2, 9, 11).half()), "float32 tensors expected"),
        ("warp odd pair", WarpDiffNormCat(), (_t(2, 5, 9, 11), _t(2, 2, 9, 11)), "two images"),
        ("chnorm rank", ChannelNorm(), (_t(3, 9, 11),), "4-D"),
        ("upsample factor", ConvexUpsample(3), (_t(2, 2, 9, 11), _t(2, 81, 9, 11)), "factor 3 is not 2, 4 or 8"),
        ("upsample mask channels", ConvexUpsample(4), (_t(2, 2, 9, 11), _t(2, 143, 9, 11)), "expected 9 \\* factor\\^2"),
        ("upsample flow channels", ConvexUpsample(2), (_t(2, 5, 9, 11), _t(2, 36, 9, 11)), "5 channels"),
        ("splat flow channels", ForwardWarp(), (_t(2, 3, 9, 11), _t(2, 3, 9, 11)), "expected 2"),
        ("splat half", ForwardWarp(), (_t(2, 3, 9, 11).half(), _t(2, 2, 9, 11).half()), "must be float32"),
        # (the operator itself: through the door the binding's own check would raise the same words on any commit)
        ("census max_distance", lambda a, b: torch.ops.fn2.census(a, b, 4, 255.0, True), (_t(2, 3, 9, 11), _t(2, 3, 9, 11)),
         "fn2::census: max_distance 4 is not 1, 2 or 3"),
        ("census channels", TernaryCensus(2), (_t(2, 2, 9, 11), _t(2, 2, 9, 11)), "expected 1 \\(grey\\) or 3"),
        ("smooth flow channels", SmoothnessLoss(2), (_t(2, 5, 9, 11), _t(2, 3, 9, 11)), "expected 1 to 4"),
        ("smooth image grad", SmoothnessLoss(2), (_t(2, 2, 9, 11, grad=True), _t(2, 3, 9, 11, grad=True)), "image requires a gradient"),
    ]


REFUSAL_IDS = ["corr rank", "corr shapes", "corr empty output", "corr stride", "fused redir", "corr1d direction", "corr1d empty output",
               "lookup radius", "lookup channels", "lookup half", "lookup coords grad", "resample flow channels", "resample half", "warp odd pair",
               "chnorm rank", "upsample factor", "upsample mask channels", "upsample flow channels", "splat flow channels", "splat half",
               "census max_distance", "census channels", "smooth flow channels", "smooth image grad"]


@pytest.mark.parametrize("which", REFUSAL_IDS)
def test_refused_at_trace_time(which):
    rows = {r[0]: r for r in _refusals()}
    assert sorted(rows) == sorted(REFUSAL_IDS)
    _, fn, args, match = rows[which]
    with pytest.raises(Exception, match=match):
        _compile(fn)(*args)


def test_backward_operator_is_not_differentiable_twice():
    """A backward operator's own autograd formula raises: create_graph=True cannot return a wrong second derivative."""
    import networks.correlation_package.correlation  # noqa: F401
    a, go = _t(2, 4, 9, 11, grad=True), _t(2, 9, 9, 11, grad=True)
    g1, _ = torch.ops.fn2.correlation_backward(a, a, go, 3, 1, 3, 1, 2, 1)
    assert g1.requires_grad
    with pytest.raises(RuntimeError, match="not differentiable a second time"):
        g1.sum().backward()


# ------------------------------------------------------------------ 6
_ISOLATION = r"""
import sys, importlib
import torch
import fn2_ops
ROWS = [("networks.correlation_package.correlation", "correlation_cuda", ["correlation", "correlation_leakyrelu_cat"]),
        ("networks.correlation_package.correlation1d", "correlation1d_cuda", ["correlation1d"]),
        ("networks.correlation_package.corr_lookup", "corr_lookup_cuda", ["corr_lookup"]),
        ("networks.resample2d_package.resample2d", "resample2d_cuda", ["resample2d", "warp_diff_norm", "warp_diff_norm_cat"]),
        ("networks.channelnorm_package.channelnorm", "channelnorm_cuda", ["channelnorm"]),
        ("networks.upsample_package.convex_upsample", "convex_upsample_cuda", ["convex_upsample"]),
        ("networks.splat_package.forward_warp", "forward_warp_cuda", ["forward_warp"]),
        ("networks.census_package.census", "census_cuda", ["census"]),
        ("networks.smoothness_package.smoothness", "smoothness_cuda", ["smoothness"]),
        ("losses_fused", "multiscale_loss_cuda", ["multiscale_loss"])]
order = [int(i) for i in sys.argv[1].split(",")]
assert fn2_ops.names() == []
ext = lambda: {m for m in sys.modules if m.endswith("_cuda")}
for i in order:
    module, extension, ops = ROWS[i]
    before_ops, before_ext = set(fn2_ops.names()), ext()
    importlib.import_module(module)
    new = sorted(set(fn2_ops.names()) - before_ops)
    want = sorted("fn2::" + o + s for o in ops for s in ("", "_backward"))
    assert new == want, (module, new, want)
    assert ext() - before_ext == {extension}, (module, ext() - before_ext)
print("isolated", len(order))
"""


@pytest.mark.parametrize("order", ["0,1,2,3,4,5,6,7,8,9", "9,8,7,6,5,4,3,2,1,0"], ids=["forward", "reversed"])
def test_importing_a_layer_registers_only_its_own_operators(order):
    """One child process per order: each import adds its own operators and its own extension to what the ones before it left."""
    import conftest
    env_path = [conftest.PKG, conftest.ROOT]
    code = "import sys; sys.path[:0] = %r\n" % env_path + _ISOLATION
    res = subprocess.run([sys.executable, "-c", code, order], capture_output=True, text=True)
    assert res.returncode == 0 and "isolated 10" in res.stdout, res.stderr[-2000:]


# ------------------------------------------------------------------ 7
DYNAMIC_DOORS = ["Correlation", "CorrelationLeakyReLUCat", "Correlation1d", "Resample2d", "WarpDiffNormCat", "WarpDiffNorm", "ChannelNorm",
                 "CorrLookup", "ConvexUpsample", "ForwardWarp", "census_distance", "SmoothnessLoss"]


def _resized(shape, dh, dw):
    return tuple(shape[:2]) + (shape[2] + dh, shape[3] + dw)


@pytest.mark.parametrize("door_id", DYNAMIC_DOORS)
def test_dynamic_shapes_do_not_recompile(door_id):
    door = CC.DOORS[CC.DOOR_IDS.index(door_id)]
    dtypes = [s[1] for s in door.inputs]
    torch._dynamo.reset()
    counter = CompileCounterWithBackend("aot_eager")
    fn = torch.compile(door.make(), backend=counter, fullgraph=True, dynamic=True)
    outs, frames = [], []
    for dh, dw in ((0, 0), (4, 6)):
        args = _meta_inputs(door, dtypes, [_resized(s[0], dh, dw) for s in door.inputs])
        out = fn(*args)
        torch.autograd.grad(out.sum(), [a for a in args if a.requires_grad])
        outs.append(tuple(out.shape))
        frames.append(counter.frame_count)
    assert frames[0] >= 1 and frames[1] == frames[0], (door_id, frames)
    assert outs[0] != outs[1] or outs[0] == ()


def test_unsup_recipe_dynamic_shapes_do_not_recompile():
    torch._dynamo.reset()
    counter = CompileCounterWithBackend("aot_eager")
    fn = torch.compile(CC.unsup_forward, backend=counter, fullgraph=True, dynamic=True)
    layers, frames = P.hip_layers(), []
    for H, W in ((36, 132), (44, 100)):
        t = {k: torch.empty((2, c, H, W), device=META) for k, c in (("im1", 3), ("im2", 3), ("flow12", 2), ("flow21", 2))}
        out = CC.run_unsup(fn, layers, types.MappingProxyType(t))
        assert out["flow12.grad"].shape == (2, 2, H, W)
        frames.append(counter.frame_count)
    assert frames[0] >= 1 and frames[1] == frames[0], frames


# ------------------------------------------------------------------ 8
def _multiscale_inputs(B=2, H=64, W=128):
    return [_t(B, 2, H >> k, W >> k, grad=(k != 4)) for k in (2, 3, 4, 5, 6)], _t(B, 2, H, W)


@pytest.mark.parametrize("norm", ["L1", "L2"])
def test_multiscale_traces(norm):
    from losses_fused import MultiScale
    crit = MultiScale(norm=norm)
    preds, target = _multiscale_inputs()
    loss, epe = _compile(lambda preds, target: crit(tuple(p * 1.0 for p in preds), target))(preds, target)
    assert loss.shape == epe.shape == () and loss.dtype == epe.dtype == torch.float32 and loss.requires_grad and not epe.requires_grad
    wanted = [p for p in preds if p.requires_grad]
    grads = torch.autograd.grad(loss, wanted)
    assert all(g.shape == p.shape and g.dtype == p.dtype for g, p in zip(grads, wanted))
    with pytest.raises(Exception, match="prediction 1 has shape"):
        _compile(lambda preds, target: crit(tuple(preds), target))([preds[0], preds[0]] + preds[2:], target)


def test_flownet2c_with_its_criterion_traces(flownet2c):
    from losses_fused import MultiScale
    model, crit = flownet2c[True].train(), MultiScale()

    def step(frames, target):
        return crit(model(frames), target)

    torch._dynamo.reset()
    frames, target = torch.empty(1, 3, 2, 64, 64, device=META), torch.empty(1, 2, 64, 64, device=META)
    rep = torch._dynamo.explain(step)(frames, target)
    assert rep.graph_break_count == 0 and rep.graph_count == 1, rep.break_reasons
    loss, epe = _compile(step)(frames, target)
    grads = torch.autograd.grad(loss, list(model.parameters()))
    assert loss.shape == () and all(g.shape == p.shape for g, p in zip(grads, model.parameters()))


# ------------------------------------------------------------------ 9
def test_make_fx_and_export_see_the_operators():
    """A direct call of an operator traces under ``make_fx`` and non-strict export; a Module reaches its operator through Dynamo only
    (``strict=True``): non-strict export and plain ``make_fx`` run ``XFunction.apply`` itself, the eager door to the C++ node."""
    from torch.fx.experimental.proxy_tensor import make_fx

    from networks.correlation_package.correlation import Correlation
    a = _t(2, 4, 9, 11)

    def direct(a, b):
        return torch.ops.fn2.correlation(a, b, 3, 1, 3, 1, 2, 1)

    class Direct(torch.nn.Module):
        def forward(self, a, b):
            return direct(a, b)

    def targets(graph):
        return [n.target for n in graph.nodes if n.op == "call_function"]

    assert targets(make_fx(direct, tracing_mode="fake")(a, a).graph) == [torch.ops.fn2.correlation.default]
    assert torch.ops.fn2.correlation.default in targets(torch.export.export(Direct(), (a, a)).graph)
    assert torch.ops.fn2.correlation.default in targets(torch.export.export(Correlation(3, 1, 3, 1, 2, 1), (a, a), strict=True).graph)
