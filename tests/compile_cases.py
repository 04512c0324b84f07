"""What tests/test_compile_host.py (meta tensors, no GPU) and tests/test_gpu_compile.py compile: every public door of the HIP layers as a
row of ``DOORS``, and forward-only twins of the two recipes of tests/pipelines_ref.py (``mini_raft`` and ``unsup_loss`` call ``.backward()``
inside; under ``torch.compile`` the backward stays outside the compiled function).  Test infrastructure only.

A door is ``Door(id, make, inputs)``: ``make()`` returns the callable (built once the layer's module is imported), ``inputs`` the
argument specs ``(shape, dtype, requires_grad)`` at a small ragged shape; ``variants`` lists the other dtype assignments the eager
door accepts (one dtype per argument).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import pipelines_ref as P

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
Door = namedtuple("Door", "id make inputs variants", defaults=((),))
G, N = True, False          # requires a gradient / does not


def _corr():
    from networks.correlation_package.correlation import Correlation, CorrelationFunction, CorrelationLeakyReLUCat
    return Correlation, CorrelationFunction, CorrelationLeakyReLUCat


def _warp():
    from networks.resample2d_package import resample2d
    return resample2d


def _splat(mode):
    from networks.splat_package import softsplat
    if mode in ("sum", "avg"):
        return lambda input, flow: softsplat(input, flow, None, mode)
    return lambda input, flow, metric: softsplat(input, flow, metric, mode)


def _lookup_block():
    from networks.correlation_package import AlternateCorrBlock
    return lambda fmap1, fmap2, coords: AlternateCorrBlock(fmap1, fmap2, num_levels=2, radius=3)(coords)


def _imp(path, name, *args, **kw):
    def make():
        import importlib
        obj = getattr(importlib.import_module(path), name)
        return obj(*args, **kw) if args or kw or isinstance(obj, type) else obj
    return make


def _apply(path, name, *extra):
    """``XFunction.apply(*tensors, *extra)``; the class is looked up when the door is made, outside what gets traced."""
    def make():
        import importlib
        function = getattr(importlib.import_module(path), name)
        return lambda *tensors: function.apply(*tensors, *extra)
    return make


_C, _R = "networks.correlation_package", "networks.resample2d_package.resample2d"
PAIR = (2, 8, 9, 11)        # two blocks of nothing in particular: odd sizes, more than one item
IMG, FLOW, X6 = (2, 3, 9, 11), (2, 2, 9, 11), (2, 6, 9, 11)
ALL4 = ((F16, F16), (BF16, BF16), (F64, F64))

DOORS = [
    Door("Correlation", lambda: _corr()[0](3, 1, 3, 1, 2, 1), [(PAIR, F32, G), (PAIR, F32, G)], ALL4),
    Door("CorrelationFunction.apply", _apply(_C + ".correlation", "CorrelationFunction", 3, 3, 4, 1, 2, 1), [(PAIR, F32, G), (PAIR, F32, G)]),
    Door("CorrelationLeakyReLUCat", lambda: _corr()[2](3, 1, 3, 1, 2, 0.1), [(PAIR, F32, G), (PAIR, F32, G), ((2, 5, 9, 11), F32, G)],
         ((F16,) * 3, (BF16,) * 3, (F64,) * 3)),
    Door("Correlation1d", _imp("networks.correlation_package", "Correlation1d", 4, 4, 1, 1, 0), [(PAIR, F32, G), (PAIR, F32, G)], ALL4),
    Door("Correlation1dFunction.apply", _apply(_C, "Correlation1dFunction", 2, 4, 1, 2, 1),
         [(PAIR, F32, G), (PAIR, F32, G)]),
    Door("Resample2d", lambda: _warp().Resample2d(), [(IMG, F32, G), (FLOW, F32, G)], ((BF16, BF16),)),
    Door("Resample2dFunction.apply", _apply(_R, "Resample2dFunction", 2, False), [(IMG, F32, G), (FLOW, F32, G)]),
    Door("WarpDiffNormCat", lambda: _warp().WarpDiffNormCat(), [(X6, F32, N), (FLOW, F32, G)], ((F16, F16), (BF16, BF16), (F32, BF16))),
    Door("WarpDiffNormCat-pair-grad", lambda: _warp().WarpDiffNormCat(), [(X6, F32, G), (FLOW, F32, G)], ((F16, F16), (BF16, BF16))),
    Door("WarpDiffNormCatFunction.apply", _apply(_R, "WarpDiffNormCatFunction", 20.0, True),
         [(X6, F32, N), (FLOW, F32, G)]),
    Door("WarpDiffNorm", lambda: _warp().WarpDiffNorm(), [(X6, F32, N), (FLOW, F32, G)], ((F16, F16), (BF16, BF16), (F32, BF16))),
    Door("WarpDiffNorm-pair-grad", lambda: _warp().WarpDiffNorm(), [(X6, F32, G), (FLOW, F32, G)]),
    Door("WarpDiffNormFunction.apply", _apply(_R, "WarpDiffNormFunction", True), [(X6, F32, N), (FLOW, F32, G)]),
    Door("ChannelNorm", _imp("networks.channelnorm_package.channelnorm", "ChannelNorm"), [(IMG, F32, G)], ((F16,), (BF16,), (F64,))),
    Door("ChannelNormFunction.apply", _apply("networks.channelnorm_package.channelnorm", "ChannelNormFunction", 2),
         [(IMG, F32, G)]),
    Door("CorrLookup", _imp("networks.correlation_package", "CorrLookup", 3), [(PAIR, F32, G), ((2, 8, 5, 6), F32, G), (FLOW, F32, N)]),
    Door("CorrLookupFunction.apply", _apply(_C, "CorrLookupFunction", 2, 0.5),
         [(PAIR, F32, G), ((2, 8, 5, 6), F32, G), (FLOW, F32, N)]),
    Door("AlternateCorrBlock", _lookup_block, [(PAIR, F32, G), (PAIR, F32, G), (FLOW, F32, N)]),
    Door("ConvexUpsample", _imp("networks.upsample_package", "ConvexUpsample", 4), [(FLOW, F32, G), ((2, 144, 9, 11), F32, G)],
         ((F32, F16), (F32, BF16))),
    Door("ConvexUpsampleFunction.apply", _apply("networks.upsample_package", "ConvexUpsampleFunction", 2, 1.5),
         [(FLOW, F32, G), ((2, 36, 9, 11), F32, G)]),
    Door("upsample_flow", _imp("networks.upsample_package", "upsample_flow"), [(FLOW, F32, G), ((2, 576, 9, 11), F32, G)]),
    Door("ForwardWarp", _imp("networks.splat_package", "ForwardWarp"), [(IMG, F32, G), (FLOW, F32, G)]),
    Door("ForwardWarpFunction.apply", _apply("networks.splat_package", "ForwardWarpFunction"), [(IMG, F32, N), (FLOW, F32, G)]),
    Door("softsplat-sum", lambda: _splat("sum"), [(IMG, F32, G), (FLOW, F32, G)]),
    Door("softsplat-avg", lambda: _splat("avg"), [(IMG, F32, G), (FLOW, F32, G)]),
    Door("softsplat-linear", lambda: _splat("linear"), [(IMG, F32, G), (FLOW, F32, G), ((2, 1, 9, 11), F32, G)]),
    Door("softsplat-soft", lambda: _splat("soft"), [(IMG, F32, G), (FLOW, F32, G), ((2, 1, 9, 11), F32, G)]),
    Door("range_map", _imp("networks.splat_package", "range_map"), [(FLOW, F32, G)]),
    Door("census_distance", _imp("networks.census_package", "census_distance"), [(IMG, F32, G), (IMG, F32, G)]),
    Door("CensusFunction.apply", _apply("networks.census_package", "CensusFunction", 2, 1.0, False),
         [(IMG, F32, N), (IMG, F32, G)]),
    Door("TernaryCensus", _imp("networks.census_package", "TernaryCensus", 1), [((2, 1, 9, 11), F32, G), ((2, 1, 9, 11), F32, N)]),
    Door("CensusLoss", _imp("networks.census_package", "CensusLoss", 3), [((2, 3, 17, 19), F32, G), ((2, 3, 17, 19), F32, G), ((2, 1, 17, 19), F32, N)]),
    Door("smoothness_map", _imp("networks.smoothness_package", "smoothness_map"), [(FLOW, F32, G), (IMG, F32, N)]),
    Door("SmoothnessFunction.apply", _apply("networks.smoothness_package", "SmoothnessFunction", 2, "gaussian", 10.0, 0.01),
         [(FLOW, F32, G), ((2, 1, 9, 11), F32, N)]),
    Door("EdgeAwareSmoothness", _imp("networks.smoothness_package", "EdgeAwareSmoothness", 2), [((2, 4, 9, 11), F32, G), (IMG, F32, N)]),
    Door("SmoothnessLoss", _imp("networks.smoothness_package", "SmoothnessLoss", 2), [(FLOW, F32, G), (IMG, F32, N)]),
]
DOOR_IDS = [d.id for d in DOORS]


def door_cases():
    """(door, dtypes) over the float32 row and every variant."""
    out = []
    for d in DOORS:
        out.append((d, tuple(s[1] for s in d.inputs)))
        out.extend((d, v) for v in d.variants)
    return out


def case_id(case):
    return case[0].id + "-" + "-".join(str(t).split(".")[1] for t in case[1])


# ------------------------------------------------------------------ the recipes, forward only
def mini_raft_forward(layers, t, params, fmap1, fmap2, upsample_input=None):
    """``pipelines_ref.mini_raft`` from the feature maps up to the loss: returns (loss, flows); ``params``: {name: leaf tensor}.  The
    two feature convolutions stay with the caller: fmap1.grad and fmap2.grad are results of the recipe, and a tensor made inside a
    compiled function has no gradient outside it."""
    im1, target = t["im1"], t["target"]
    N_, _, H, W = fmap1.shape
    corr_fn = layers.corr_block(fmap1, fmap2, P.RAFT_LEVELS, P.RAFT_RADIUS)
    ys, xs = torch.meshgrid(torch.arange(H, device=im1.device, dtype=im1.dtype), torch.arange(W, device=im1.device, dtype=im1.dtype),
                            indexing="ij")
    coords0 = torch.stack([xs, ys])[None].expand(N_, 2, H, W).contiguous()
    coords1 = coords0.clone()
    flows = []
    for _ in range(P.RAFT_ITERS):
        coords1 = coords1.detach()
        corr = corr_fn(coords1)
        flow = coords1 - coords0
        h = torch.tanh(F.conv2d(torch.cat([corr, flow], 1), params["update.weight"], params["update.bias"], padding=1))
        coords1 = coords1 + F.conv2d(h, params["delta.weight"], params["delta.bias"], padding=1)
        up_mask = 0.25 * F.conv2d(h, params["mask.weight"], params["mask.bias"])
        flow = coords1 - coords0
        flows.append(layers.upsample(upsample_input(flow) if upsample_input else flow, up_mask))
    loss = sum(0.8 ** (P.RAFT_ITERS - 1 - i) * (f - target).abs().mean() for i, f in enumerate(flows))
    return loss, tuple(flows)


def unsup_forward(layers, im1, im2, flow12, flow21):
    """``pipelines_ref.unsup_loss`` up to the loss: returns (loss, photometric, smooth, noc)."""
    im2_warped = layers.warp(im2, flow12.contiguous())
    noc = (layers.range_map(flow21) > 0.5).to(im1.dtype)
    photometric = layers.census(im1, im2_warped, noc)
    flow12_quarter = 0.25 * F.avg_pool2d(flow12, 4)
    im1_quarter = F.avg_pool2d(im1, 4)
    smooth = layers.smooth(flow12_quarter, im1_quarter.detach())
    loss = photometric + 4.0 * smooth
    return loss, photometric, smooth, noc


def run_mini_raft(fn, layers, t, context=None, upsample_input=None):
    """``fn`` = ``mini_raft_forward`` or its compiled twin; the backward outside it.  The dictionary of ``pipelines_ref.mini_raft``."""
    import contextlib
    params = {k: t[k].detach().clone().requires_grad_(True) for k in P.RAFT_PARAMS}
    with (context or contextlib.nullcontext)():
        fmap1 = F.conv2d(t["im1"] - 0.5, params["fnet.weight"], params["fnet.bias"], stride=8)
        fmap2 = F.conv2d(t["im2"] - 0.5, params["fnet.weight"], params["fnet.bias"], stride=8)
        loss, flows = fn(layers, t, params, fmap1, fmap2, upsample_input)
    names = list(params)
    grads = torch.autograd.grad(loss, [fmap1, fmap2] + [params[k] for k in names])
    out = {"flow_up_%d" % i: f.detach() for i, f in enumerate(flows)}
    out.update({"loss": loss.detach(), "fmap1.grad": grads[0], "fmap2.grad": grads[1]})
    out.update({k + ".grad": g for k, g in zip(names, grads[2:])})
    return out


def run_unsup(fn, layers, t):
    """``fn`` = ``unsup_forward`` or its compiled twin; the backward outside it.  The dictionary of ``pipelines_ref.unsup_loss``."""
    im1, im2, flow12 = (t[k].detach().clone().requires_grad_(True) for k in ("im1", "im2", "flow12"))
    loss, photometric, smooth, noc = fn(layers, im1, im2, flow12, t["flow21"])
    loss.backward()
    return {"loss": loss.detach(), "photometric": photometric.detach(), "smooth": smooth.detach(), "noc": noc.detach(),
            "im1.grad": im1.grad, "im2.grad": torch.zeros_like(im2) if im2.grad is None else im2.grad, "flow12.grad": flow12.grad}


def make_inputs(door, dtypes, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for (shape, _, need), dtype in zip(door.inputs, dtypes):
        t = torch.randn(shape, generator=g).to(dtype)
        out.append(t.to(device).requires_grad_(need))
    return out
