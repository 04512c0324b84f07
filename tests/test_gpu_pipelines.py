"""The newer layers the way a model runs them: composed, through autograd, over several iterations, under autocast, under the
deterministic flag and inside a hipGraph -- the two recipes INTEGRATION.md prints (tests/pipelines_ref.py), on the HIP modules,
against the same recipes composed in PyTorch in float64.

Acceptance rule for a composed tensor T (``pipelines_ref.rule_bound``):

    max |T_hip - T_64|  <=  max(8 max |T_32 - T_64|, 2^-20 max |T_64|)

with T_32 the float32 PyTorch composition, evaluated here on the GPU.  The rule is measured against the reference composition,
never against the code under test; tests/test_pipelines_host.py shows that every wiring mutation misses it by orders of magnitude.

a. AlternateCorrBlock's backward per element, against bounds derived from the header's (not measured);
b. mini-RAFT on the HIP layers by the rule; a second run repeats the bits of everything upstream of grad_fmap2's atomics;
c. mini-RAFT under autocast (float16, bfloat16) as INTEGRATION.md instructs;
d. the unsupervised loss on the HIP layers by the rule, the occlusion mask bit for bit;
e. the deterministic flag: the unsupervised loss repeats its bits, mini-RAFT's backward raises (warns with warn_only);
f. hipGraph replay of both recipes and of the remaining new layers, on fresh input values in the captured buffers.

This file goes through the modules only; the C-ABI-level guards (NaN prefill, sentinels) are the per-layer tests'."""
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_contract_ref as R
import corr_lookup_ref as RL
import forward_warp_ref as FR
import pipelines_ref as P
from test_gpu_corr_lookup import _coords, _features

pytestmark = pytest.mark.gpu

# what lies downstream of a float atomic, and so repeats to rounding only
RAFT_AFTER_ATOMICS = ("fmap2.grad", "fnet.weight.grad", "fnet.bias.grad")      # CorrLookup's grad_fmap2
UNSUP_AFTER_ATOMICS = ("im2.grad",)                                             # Resample2d's grad_input1

_REFERENCES = {}


def reference(recipe, seed, dev):
    """(inputs, float64 composition, float32 composition) of a recipe, computed once per seed and shared."""
    if (recipe, seed) not in _REFERENCES:
        pipeline, inputs = {"raft": (P.mini_raft, P.raft_inputs), "unsup": (P.unsup_loss, P.unsup_inputs)}[recipe]
        inp = inputs(seed)
        _REFERENCES[recipe, seed] = (inp, P.run(pipeline, inp, torch.float64, dev), P.run(pipeline, inp, torch.float32, dev))
    return _REFERENCES[recipe, seed]


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, by up to {float((a - b).abs().max()):.3g}"


def by_the_rule(got, o32, o64, what, keys=None):
    keys = list(o64) if keys is None else keys
    misses = P.rule_misses({k: got[k] for k in keys}, o32, {k: o64[k] for k in keys}, what + " ")
    assert not misses, f"{what}: {misses} miss the rule"


class Recorder:
    """The layers of ``inner``, recording every lookup and every upsampling with what they were given, what they returned, the
    mask's gradient (``retain_grad``) and the gradient that arrives at the upsampled flow."""

    def __init__(self, inner):
        self.lookups, self.upsamples = [], []

        def corr_block(fmap1, fmap2, num_levels, radius):
            fn = inner.corr_block(fmap1, fmap2, num_levels, radius)

            def lookup(coords):
                out = fn(coords)
                self.lookups.append(dict(fmap1=fmap1, fmap2=fmap2, coords=coords, out=out))
                return out
            return lookup

        def upsample(flow, mask):
            mask.retain_grad()
            rec = dict(flow=flow, mask=mask, out=inner.upsample(flow, mask))
            rec["out"].register_hook(lambda g: rec.__setitem__("grad_out", g))
            self.upsamples.append(rec)
            return rec["out"]

        self.layers = types.SimpleNamespace(**{**vars(inner), "corr_block": corr_block, "upsample": upsample})


# ------------------------------------------------------------------ a: AlternateCorrBlock's backward, per element
def _adjoint(t, times):
    """avg_pool2d(2, 2)'s adjoint ``times`` times: every fine pixel gets a quarter of its coarse pixel (even sizes)."""
    for _ in range(times):
        t = 0.25 * np.repeat(np.repeat(t, 2, axis=2), 2, axis=3)
    return t


def test_alternate_corr_block_backward_per_element(dev):
    """2 x 16 x 24 x 32, 3 levels, r = 3, the forward test's inputs, grad_output normal; the reference is the float64 gradient of
    corr_lookup_ref.compose(num_levels=3), which pools the all-pairs volume as RAFT does.

    The layer is  cat_i lookup(fmap1, P^i fmap2, coords / 2^i)  with P = avg_pool2d(2, 2); autograd gives
        fmap1.grad = sum_i g1_i,          fmap2.grad = sum_i (P^T)^i g2_i
    with g1_i, g2_i the two gradients of level i's lookup, which the header bounds per element.

    fmap1.grad: the sum over the levels of the header's bound, delta_grad1 of level i with S from the float64-pooled fmap2.  Not in
    it: the layer pools fmap2 in fp32 (3 adds and a product per level of pooling, relative to the pooled |fmap2|) and autograd adds
    the three levels in fp32 (2 adds) -- a few 2^-24 of sums the bound already holds (4 r + 13) 2^-23 of, with its factor of two
    in hand.  coords / 2^i is exact.

    fmap2.grad: P^T has the non-negative weights 1/4, so |(P^T)^i (g - exact)| <= (P^T)^i delta_grad2_i: the level bounds map
    through the same adjoint and add.  On top, in fp32: each of the L - 1 adjoints (a product with 1/4: exact, counted all the
    same) and each of the L - 1 additions of autograd's accumulation is one 2^-24 relative step on the sum of the magnitudes
    that meet there, at most M = sum_i (P^T)^i (|exact_i| + delta_i): 2 (L - 1) 2^-24 M.  grad_fmap2 does not depend on fmap2,
    so the fp32 pooling does not enter.  Where no term of any level arrives the bound is 0: the gradient is exactly zero."""
    from networks.correlation_package import AlternateCorrBlock
    B, C, H, W, r, L = 2, 16, 24, 32, 3, 3
    D2 = (2 * r + 1) ** 2
    f1, f2 = _features(1, C, (H, W), (H, W), seed=9)
    co = _coords("a", B, H, W, H, W, r, seed=10)
    go = R.grad_output("normal", (B, L * D2, H, W), seed=11)
    scale = float(C) ** -0.5
    a, b = f1.to(dev).requires_grad_(True), f2.to(dev).requires_grad_(True)
    AlternateCorrBlock(a, b, num_levels=L, radius=r)(co.to(dev)).backward(go.to(dev))
    a64, b64 = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    RL.compose(a64, b64, co.double(), r, scale, num_levels=L).backward(go.double())
    want1, want2 = a64.grad.numpy(), b64.grad.numpy()
    bound1, bound2, mag2 = np.zeros((B, C, H, W)), np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    sum1, sum2, terms = np.zeros((B, C, H, W)), np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    lvl = f2.double()
    for i in range(L):
        if i:
            lvl = F.avg_pool2d(lvl, 2, stride=2)
        (g1, S1), (g2, S2, n2) = RL.backward(f1.numpy(), lvl.numpy(), (co / 2 ** i).numpy(), go[:, i * D2:(i + 1) * D2].numpy(), r, scale)
        bound1 += RL.delta_grad1(g1, S1, r, scale)
        d2 = RL.delta_grad2(g2, S2, n2, scale)
        bound2 += _adjoint(d2, i)
        mag2 += _adjoint(np.abs(g2) + d2, i)
        sum1, sum2, terms = sum1 + g1, sum2 + _adjoint(g2, i), terms + _adjoint(n2.astype(np.float64), i)
    # the decomposition is the reference: level by level it adds up to the composition's gradient (the fp32 fraction of the
    # header differs from the exact one by 2^-25 for -1 < c < 0 only)
    assert np.abs(sum1 - want1).max() <= 1e-6 * np.abs(want1).max() and np.abs(sum2 - want2).max() <= 1e-6 * np.abs(want2).max()
    bound2 += 2 * (L - 1) * 2.0 ** -24 * mag2
    for name, got, want, bound in (("fmap1.grad", a.grad, want1, bound1), ("fmap2.grad", b.grad, want2, bound2)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f"  AlternateCorrBlock {name}: error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}  (scale {np.abs(want).max():.3g})")
        assert (err <= bound).all(), name
        assert np.abs(want).max() > 0.1
    none = terms == 0
    assert (b.grad.cpu().numpy()[none] == 0).all() and (want2[none] == 0).all()


def test_alternate_corr_block_backward_one_pixel_grad_output(dev):
    """Which level and channel a gradient lands in: grad_output is 1 at one channel of one level at pixel (y, x) = (8, 12) and 0
    elsewhere, the coordinates are the integer identity.  Level l looks from (12, 8) / 2^l -- an integer position -- so channel
    i D + j is the single tap at level-l pixel (12 / 2^l + i - r, 8 / 2^l + j - r) with weight 1:
      fmap2.grad = fl32(scale * fmap1[0, :, 8, 12]) / 4^l on that pixel's 2^l x 2^l block (the grid weight is scale exactly, the
                   product is one rounding, the adjoint's quarters are exact), and exactly 0 everywhere else;
      fmap1.grad = fl32(scale * (the layer's level-l fmap2 at that pixel)) at (8, 12) and exactly 0 everywhere else."""
    from networks.correlation_package import AlternateCorrBlock
    B, C, H, W, r, L = 1, 16, 24, 32, 3, 3
    D, y, x = 2 * r + 1, 8, 12
    f1, f2 = _features(1, C, (H, W), (H, W), seed=9, B=B)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ident = torch.stack([xs, ys])[None].to(dev)
    scale = torch.tensor(float(C) ** -0.5, dtype=torch.float32, device=dev)
    for lvl, (i, j) in enumerate([(r + 2, r - 1), (r - 3, r + 1), (r + 1, r + 3)]):
        a, b = f1.to(dev).requires_grad_(True), f2.to(dev).requires_grad_(True)
        block = AlternateCorrBlock(a, b, num_levels=L, radius=r)
        go = torch.zeros(B, L * D * D, H, W, device=dev)
        go[0, lvl * D * D + i * D + j, y, x] = 1.0
        block(ident).backward(go)
        tx, ty = (x >> lvl) + i - r, (y >> lvl) + j - r
        assert 0 <= tx < (W >> lvl) and 0 <= ty < (H >> lvl)
        want2 = torch.zeros_like(b)
        want2[0, :, ty << lvl:(ty + 1) << lvl, tx << lvl:(tx + 1) << lvl] = (scale * a.detach()[0, :, y, x] * 0.25 ** lvl)[:, None, None]
        same_bits(b.grad, want2, f"level {lvl} fmap2.grad")
        want1 = torch.zeros_like(a)
        want1[0, :, y, x] = scale * block.pyramid[lvl].detach()[0, :, ty, tx]
        same_bits(a.grad, want1, f"level {lvl} fmap1.grad")
        assert float(want1.abs().max()) > 0 and float(want2.abs().max()) > 0
        pooled = f2.double()
        for _ in range(lvl):
            pooled = F.avg_pool2d(pooled, 2, stride=2)
        assert float((block.pyramid[lvl].detach().cpu().double() - pooled).abs().max()) <= 4 * lvl * 2.0 ** -24 * float(f2.abs().max())


# ------------------------------------------------------------------ b: mini-RAFT on the HIP layers
def test_mini_raft_on_the_hip_layers(dev):
    """By the rule, with the convolution algorithms a user gets by default; then two more runs from the same state, which must
    repeat the bits of everything upstream of grad_fmap2's atomics.  The recipe's convolutions are MIOpen's, whose weight
    gradients do not repeat their bits by default (outside this project); that pair alone asks the backend for its
    deterministic algorithms, so that what is left to differ is the layers'."""
    inp, o64, o32 = reference("raft", 0, dev)
    t = P._cast(inp, torch.float32, dev)
    rec = Recorder(P.hip_layers())
    got = P.mini_raft(rec.layers, t)
    assert len(rec.lookups) == len(rec.upsamples) == P.RAFT_ITERS
    for u in rec.upsamples:
        assert u["out"].dtype == torch.float32 and u["out"].is_contiguous() and u["out"].shape == (P.RAFT_SHAPE[0], 2) + P.RAFT_SHAPE[1:]
    by_the_rule(got, o32, o64, "mini-RAFT on the HIP layers")
    before = torch.backends.cudnn.deterministic
    try:
        torch.backends.cudnn.deterministic = True
        first, again = P.mini_raft(P.hip_layers(), t), P.mini_raft(P.hip_layers(), t)
    finally:
        torch.backends.cudnn.deterministic = before
    differ = [k for k in first if k not in RAFT_AFTER_ATOMICS and not torch.equal(again[k], first[k])]
    assert not differ, f"second run: {differ} do not repeat their bits"
    for k in RAFT_AFTER_ATOMICS:
        assert float((again[k] - first[k]).abs().max()) <= P.rule_bound(o32[k], o64[k]), k
    by_the_rule(first, o32, o64, "mini-RAFT on the HIP layers, deterministic convolutions")


# ------------------------------------------------------------------ c: mini-RAFT under autocast
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_mini_raft_under_autocast(dev, dtype):
    """"Under autocast pass flow.float(); the mask may stay in half or bfloat16 and gets its gradient in that type."
    The convolutions run in the 16-bit type; every custom call inside the region must have the bits of the same call made
    outside it on the exactly widened inputs."""
    from networks.correlation_package import AlternateCorrBlock
    from networks.upsample_package import upsample_flow
    t = P._cast(P.raft_inputs(0), torch.float32, dev)
    rec = Recorder(P.hip_layers())
    got = P.mini_raft(rec.layers, t, upsample_input=lambda f: f.float(), context=lambda: torch.autocast("cuda", dtype=dtype))
    assert len(rec.lookups) == len(rec.upsamples) == P.RAFT_ITERS
    for n, c in enumerate(rec.lookups):
        assert c["fmap1"].dtype == c["fmap2"].dtype == dtype, "the feature convolution did not run in the 16-bit type"
        assert c["out"].dtype == torch.float32
        with torch.no_grad():
            outside = AlternateCorrBlock(c["fmap1"].float(), c["fmap2"].float(), num_levels=P.RAFT_LEVELS, radius=P.RAFT_RADIUS)(c["coords"].float())
        same_bits(c["out"].detach(), outside, f"lookup {n} inside the region")
    for n, u in enumerate(rec.upsamples):
        flow, mask = u["flow"].detach(), u["mask"].detach()
        assert flow.dtype == torch.float32 and mask.dtype == dtype and u["out"].dtype == torch.float32
        with torch.no_grad():
            same_bits(u["out"].detach(), upsample_flow(flow, mask), f"upsampling {n}, the 16-bit mask outside the region")
            same_bits(u["out"].detach(), upsample_flow(flow, mask.float()), f"upsampling {n}, the widened mask")
        f, m = flow.clone().requires_grad_(True), mask.float().requires_grad_(True)
        upsample_flow(f, m).backward(u["grad_out"])
        assert u["mask"].grad is not None and u["mask"].grad.dtype == dtype
        same_bits(u["mask"].grad, m.grad.to(dtype), f"upsampling {n}, mask.grad = the float32 gradient rounded once")
        assert float(m.grad.abs().max()) > 0
    for k in P.RAFT_PARAMS:
        g = got[k + ".grad"]
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    assert bool(torch.isfinite(got["loss"])) and got["loss"].dtype == torch.float32
    u = rec.upsamples[0]
    with torch.autocast("cuda", dtype=dtype), pytest.raises(RuntimeError, match=r"flow must be float32.*\.float\(\)"):
        upsample_flow(u["flow"].detach().to(dtype), u["mask"].detach())


# ------------------------------------------------------------------ d: the unsupervised loss on the HIP layers
def _two_terms_of_the_flow_gradient(inp, dev):
    """flow12.grad of the float64 composition, split: (through the warp and the census term, through the regulariser)."""
    t = P._cast(inp, torch.float64, dev)
    ref = P.torch_layers()
    photo = types.SimpleNamespace(**{**vars(ref), "smooth": lambda flow, image: flow.sum() * 0})
    smooth = types.SimpleNamespace(**{**vars(ref), "census": lambda im1, im2_warped, mask: im2_warped.sum() * 0})
    return P.unsup_loss(photo, t)["flow12.grad"], P.unsup_loss(smooth, t)["flow12.grad"]


def test_unsupervised_loss_on_the_hip_layers(dev):
    inp, o64, o32 = reference("unsup", 0, dev)
    P.check_unsup_inputs(inp)
    got = P.run(P.unsup_loss, inp, torch.float32, dev, layers=P.hip_layers())
    assert got["noc"].dtype == torch.float32
    same_bits(got["noc"].double(), o64["noc"], "noc against float64")
    same_bits(o32["noc"].double(), o64["noc"], "float32's noc against float64")
    from networks.splat_package import range_map
    rm = range_map(P._cast(inp, torch.float32, dev)["flow21"])
    assert torch.equal(4 * rm, (4 * rm).round()) and 0.2 <= float(got["noc"].mean()) <= 0.9
    by_the_rule(got, o32, o64, "unsupervised loss on the HIP layers")
    # both custom nodes reach the leaf flow12.  Every pixel lies under a regulariser stencil (36 x 132 is four times 9 x 33), so
    # "only the warp" means: the regulariser's share is below the rule's bound for this tensor, the warp's far above it
    g_warp, g_reg = _two_terms_of_the_flow_gradient(inp, dev)
    g64 = o64["flow12.grad"]
    bound = P.rule_bound(o32["flow12.grad"], g64)
    assert float((g_warp + g_reg - g64).abs().max()) <= 1e-12 * float(g64.abs().max())
    only_reg = (g_warp == 0) & (g_reg.abs() > 4 * bound)
    only_warp = (g_reg.abs() <= bound) & (g_warp.abs() > 64 * bound)
    print(f"  flow12.grad: {int(only_reg.sum())} elements with the regulariser only, {int(only_warp.sum())} with the warp only; "
          f"largest share of the regulariser {float(g_reg.abs().max()):.3g}, of the warp {float(g_warp.abs().max()):.3g}")
    assert int(only_reg.sum()) >= 8 and int(only_warp.sum()) >= 8
    g = got["flow12.grad"].double()
    for where in (only_reg, only_warp):
        assert bool((g[where] != 0).all())
        assert float((g[where] - g64[where]).abs().max()) <= bound


# ------------------------------------------------------------------ e: the deterministic flag
def test_deterministic_flag(dev):
    """Under torch.use_deterministic_algorithms(True), with warnings as errors: the unsupervised recipe -- Resample2d's fixed-point
    scatter, ForwardWarp's fixed-point splat, census and smoothness without atomics -- gives identical bits in the loss and all
    three gradients three times over and once more on a side stream, and still meets the rule; mini-RAFT's backward raises the
    documented corr_lookup_cuda.backward error (grad_fmap2 is a float-atomic scatter) and warns with warn_only=True."""
    inp, o64, o32 = reference("unsup", 0, dev)
    t = P._cast(inp, torch.float32, dev)
    traft = P._cast(P.raft_inputs(0), torch.float32, dev)
    hip = P.hip_layers()
    keys = ("loss", "photometric", "smooth", "noc", "im1.grad", "im2.grad", "flow12.grad")
    try:
        torch.use_deterministic_algorithms(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            runs = [P.unsup_loss(hip, t) for _ in range(3)]
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                runs.append(P.unsup_loss(hip, t))
            side.synchronize()
            torch.cuda.synchronize()
            with pytest.raises(RuntimeError, match="corr_lookup_cuda.backward"):
                P.mini_raft(hip, traft)
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.warns(UserWarning, match="corr_lookup_cuda.backward"):
            warned = P.mini_raft(hip, traft)
    finally:
        torch.use_deterministic_algorithms(False)
    for n, other in enumerate(runs[1:], 1):
        for k in keys:
            same_bits(other[k], runs[0][k], f"run {n} ({'side stream' if n == 3 else 'same stream'}), {k}")
    by_the_rule(runs[0], o32, o64, "unsupervised loss under the deterministic flag")
    assert bool(torch.isfinite(warned["loss"]))


# ------------------------------------------------------------------ f: hipGraph replay
def _capture(step):
    """The pattern of tests/test_gpu_streams.py: three warm-up runs on a side stream, then the capture."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    return graph, captured


def _replay(graph, captured, static, fresh):
    with torch.no_grad():
        for k, v in static.items():
            v.copy_(fresh[k])
    graph.replay()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in captured.items()}


@pytest.mark.parametrize("recipe", ["unsup", "raft"])
def test_recipe_replays_from_a_hip_graph(dev, recipe):
    """Forward and backward of a recipe captured into one hipGraph -- the layers' hipMemsetAsync zero fills and their workspaces
    from the caching allocator included -- and replayed on two fresh sets of input values copied into the captured buffers.
    Bit for bit the eager run on those values wherever no float atomic lies upstream (the whole unsupervised loss except
    im2.grad; mini-RAFT's flow_up); everything against float64 by the rule of b and d."""
    pipeline, inputs, after = {"unsup": (P.unsup_loss, P.unsup_inputs, UNSUP_AFTER_ATOMICS),
                               "raft": (P.mini_raft, P.raft_inputs, RAFT_AFTER_ATOMICS)}[recipe]
    hip = P.hip_layers()
    static = P._cast(inputs(0), torch.float32, dev)
    graph, captured = _capture(lambda: pipeline(hip, static))
    for seed in (1, 2):
        inp, o64, o32 = reference(recipe, seed, dev)
        if recipe == "unsup":
            P.check_unsup_inputs(inp)
            assert 0.2 <= float(o64["noc"].mean()) <= 0.9
        fresh = P._cast(inp, torch.float32, dev)
        got = _replay(graph, captured, static, fresh)
        eager = pipeline(hip, fresh)
        torch.cuda.synchronize()
        exact = [k for k in got if k not in after] if recipe == "unsup" else ["flow_up_%d" % i for i in range(P.RAFT_ITERS)]
        for k in exact:
            same_bits(got[k], eager[k], f"seed {seed}, replay against eager, {k}")
        by_the_rule(got, o32, o64, f"{recipe} replayed, seed {seed}")


def _softsplat_composition(x, flow, metric):
    w = metric.exp()
    out = FR.compose(torch.cat([x * w, w], 1), flow)
    return out[:, :-1] / (out[:, -1:] + 1e-7)


def _small_inputs(seed, dev):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(a1=r(2, 20, 9, 70), b1=r(2, 20, 9, 70), go1=r(2, 9, 9, 70), a2=r(2, 20, 17, 70), b2=r(2, 20, 17, 70), go2=r(2, 81, 17, 70),
             x=r(2, 3, 17, 67), metric=0.5 * r(2, 1, 17, 67), go3=r(2, 3, 17, 67), x4=r(2, 3, 17, 67), go4=r(2, 3, 17, 67))
    d["flow"] = torch.from_numpy(FR.flow_family("smooth", 2, 17, 67, seed=seed))
    d["flow4"] = torch.from_numpy(FR.flow_family("smooth", 2, 17, 67, seed=seed + 100))
    return {k: v.to(dev) for k, v in d.items()}


SMALL_LEAVES = ("a1", "b1", "a2", "b2", "x", "flow", "metric", "x4", "flow4")
SMALL_AFTER_ATOMICS = ("softsplat", "x.grad", "flow.grad", "metric.grad")      # the splat's float atomics, and what reads its output


def _small_step(t, splat=None, warp=None, only_splat=False):
    """Forward and backward of the remaining new layers at small ragged shapes: Correlation1d(4, 4, 1, 1), Correlation(4, 1, 4,
    1, 1), softsplat(mode="soft") and ForwardWarp under the deterministic flag."""
    from networks.correlation_package.correlation import Correlation
    from networks.correlation_package.correlation1d import Correlation1d
    from networks.splat_package import ForwardWarp, softsplat
    leaf = {k: t[k].detach().clone().requires_grad_(True) for k in SMALL_LEAVES}
    out = {"softsplat": (splat or (lambda x, f, m: softsplat(x, f, m, mode="soft")))(leaf["x"], leaf["flow"], leaf["metric"])}
    loss = (out["softsplat"] * t["go3"]).sum()
    if not only_splat:
        out["corr1d"] = Correlation1d(4, 4, 1, 1)(leaf["a1"], leaf["b1"])
        out["corr"] = Correlation(4, 1, 4, 1, 1)(leaf["a2"], leaf["b2"])
        try:
            torch.use_deterministic_algorithms(True)
            out["forward_warp"] = ForwardWarp()(leaf["x4"], leaf["flow4"])
        finally:
            torch.use_deterministic_algorithms(False)
        loss = loss + (out["corr1d"] * t["go1"]).sum() + (out["corr"] * t["go2"]).sum() + (out["forward_warp"] * t["go4"]).sum()
    loss.backward()
    out = {k: v.detach() for k, v in out.items()}
    out.update({k + ".grad": v.grad for k, v in leaf.items() if v.grad is not None})
    return out


def test_remaining_layers_replay_from_a_hip_graph(dev):
    """One graph with the layers neither recipe holds.  Bit for bit the eager run everywhere except the non-deterministic splat
    forward and the three gradients that read its output; those against the float64 composition by the rule."""
    static = _small_inputs(40, dev)
    graph, captured = _capture(lambda: _small_step(static))
    assert set(captured) == {"softsplat", "corr1d", "corr", "forward_warp"} | {k + ".grad" for k in SMALL_LEAVES}
    for seed in (41, 42):
        fresh = _small_inputs(seed, dev)
        got = _replay(graph, captured, static, fresh)
        eager = _small_step(fresh)
        torch.cuda.synchronize()
        for k in got:
            assert float(got[k].abs().max()) > 0, k
            if k not in SMALL_AFTER_ATOMICS:
                same_bits(got[k], eager[k], f"seed {seed}, replay against eager, {k}")
        o64 = _small_step({k: v.double() for k, v in fresh.items()}, splat=_softsplat_composition, only_splat=True)
        o32 = _small_step(fresh, splat=_softsplat_composition, only_splat=True)
        by_the_rule(got, o32, o64, f"softsplat replayed, seed {seed}", keys=list(SMALL_AFTER_ATOMICS))
