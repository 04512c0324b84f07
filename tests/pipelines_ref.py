"""The two recipes INTEGRATION.md prints for the newer layers, as functions of their layers -- a RAFT refinement loop
(``AlternateCorrBlock`` + ``upsample_flow``) and a UFlow-style unsupervised loss (``Resample2d``, ``range_map``, ``CensusLoss``,
``SmoothnessLoss``) -- with the PyTorch compositions of those layers in any dtype, the inputs, the acceptance rule and the wiring
mutations of tests/test_pipelines_host.py.  Test infrastructure only.

A pipeline takes a ``Layers`` object, so one function runs on the compositions (``torch_layers()``: float64 is the reference,
float32 the yardstick of the rule) or on the HIP modules (``hip_layers()``).  The compositions are the ``compose`` functions of
the per-layer reference modules; the only new one is ``gather_warp``, the backward warp.

Acceptance rule for a composed tensor T:

    max |T_hip - T_64|  <=  max(8 max |T_32 - T_64|, 2^-20 max |T_64|)

Both sides evaluate one function in float32 with different summation orders, hence a small factor; the floor of 16 half-ulps at
the tensor's scale is there because a scalar's float32 error can be small by luck.
"""
import contextlib
import types

import numpy as np
import torch
import torch.nn.functional as F

import census_ref as CR
import convex_upsample_ref as UR
import corr_lookup_ref as RL
import forward_warp_ref as FR
import smoothness_ref as SR

RULE_FACTOR = 8.0
RULE_FLOOR = 2.0 ** -20

MUTATIONS_RAFT = ("levels_reversed", "coords_not_divided", "upsample_scale_1", "coords_not_detached")
MUTATIONS_UNSUP = ("noc_inverted", "flow_channels_swapped", "im1_warped", "order_1", "full_resolution_image_cropped")


# ------------------------------------------------------------------ the rule
def _np64(t):
    return t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def rule_bound(t32, t64):
    t32, t64 = _np64(t32), _np64(t64)
    assert t32.shape == t64.shape, (t32.shape, t64.shape)
    return max(RULE_FACTOR * float(np.abs(t32 - t64).max()), RULE_FLOOR * float(np.abs(t64).max()))


def rule_report(got, out32, out64, what=""):
    """{name: (error, bound, error / float32's error)} over the keys of ``out64``; prints one line per tensor."""
    rep = {}
    for k, ref in out64.items():
        ref, g = _np64(ref), _np64(got[k])
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        err, e32 = float(np.abs(g - ref).max()), float(np.abs(_np64(out32[k]) - ref).max())
        rep[k] = (err, rule_bound(out32[k], ref), err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf")))
        print(f"  {what}{k}: error {err:.3g}  bound {rep[k][1]:.3g}  error / float32's {rep[k][2]:.3g}  (scale {np.abs(ref).max():.3g})")
    return rep


def rule_misses(got, out32, out64, what=""):
    """The names of the tensors that miss the rule (NaN misses)."""
    return [k for k, (err, bound, _) in rule_report(got, out32, out64, what).items() if not err <= bound]


# ------------------------------------------------------------------ the backward warp as a gather
def gather_warp(img, flow):
    """Resample2d(kernel_size=1, bilinear) in the tensors' dtype: out[b, c, y, x] = the bilinear sample of img[b, c] at
    (x + flow_x, y + flow_y).  ``floor`` is taken on a detached tensor, the corner indices are clamped into the image and the
    weights come from the unclamped fractions, so a sample outside the image reads the border pixel and autograd gives the
    reference's flow gradient there too (the clamped corners' difference), where grid_sample(padding_mode="border") gives 0."""
    B, C, H, W = img.shape
    xs = torch.arange(W, device=img.device, dtype=img.dtype)[None, None, :]
    ys = torch.arange(H, device=img.device, dtype=img.dtype)[None, :, None]
    xf, yf = xs + flow[:, 0], ys + flow[:, 1]
    x0, y0 = xf.detach().floor(), yf.detach().floor()
    ax, ay = (xf - x0)[:, None], (yf - y0)[:, None]
    xl, xr = x0.long().clamp(0, W - 1), (x0.long() + 1).clamp(0, W - 1)
    yt, yb = y0.long().clamp(0, H - 1), (y0.long() + 1).clamp(0, H - 1)
    flat = img.reshape(B, C, H * W)

    def at(yy, xx):
        return flat.gather(2, (yy * W + xx).reshape(B, 1, H * W).expand(B, C, H * W)).reshape(B, C, H, W)

    return (1 - ax) * (1 - ay) * at(yt, xl) + ax * (1 - ay) * at(yt, xr) + (1 - ax) * ay * at(yb, xl) + ax * ay * at(yb, xr)


# ------------------------------------------------------------------ the layers
def torch_layers(mutation=None):
    """The PyTorch compositions, in the dtype of the tensors they are given.  ``mutation`` wires one of them wrongly (the
    mutations that live inside a layer; the others are in the pipelines)."""

    def corr_block(fmap1, fmap2, num_levels, radius):
        scale = float(fmap1.shape[1]) ** -0.5
        if mutation not in ("levels_reversed", "coords_not_divided"):
            return lambda coords: RL.compose(fmap1, fmap2, coords, radius, scale, num_levels=num_levels)
        # level by level on the pooled fmap2 (the pooling is linear: the same function as pooling the volume)
        pyramid = [fmap2]
        for _ in range(num_levels - 1):
            pyramid.append(F.avg_pool2d(pyramid[-1], 2, stride=2))

        def lookup(coords):
            out = [RL.compose(fmap1, f2, coords if mutation == "coords_not_divided" else coords / 2 ** i, radius, scale)
                   for i, f2 in enumerate(pyramid)]
            return torch.cat(out[::-1] if mutation == "levels_reversed" else out, dim=1)
        return lookup

    def upsample(flow, mask):
        return UR.compose(flow, mask.to(flow.dtype), 8, 1.0 if mutation == "upsample_scale_1" else 8.0)

    def range_map(flow):
        return FR.compose(flow.new_ones((flow.shape[0], 1) + tuple(flow.shape[2:])), flow)

    def census(im1, im2_warped, mask):
        return CR.compose_loss(CR.torch_grey(im1, 255.0), CR.torch_grey(im2_warped, 255.0), mask, md=3)

    def smooth(flow, image):
        return SR.compose_loss(flow, image, 1 if mutation == "order_1" else 2, "exponential", 150.0, 0.001)

    return types.SimpleNamespace(corr_block=corr_block, upsample=upsample, warp=gather_warp, range_map=range_map, census=census,
                                 smooth=smooth)


def hip_layers():
    """The HIP modules, called as INTEGRATION.md prints them."""
    from networks.census_package import CensusLoss
    from networks.correlation_package import AlternateCorrBlock
    from networks.resample2d_package.resample2d import Resample2d
    from networks.smoothness_package import SmoothnessLoss
    from networks.splat_package import range_map
    from networks.upsample_package import upsample_flow
    return types.SimpleNamespace(
        corr_block=lambda fmap1, fmap2, num_levels, radius: AlternateCorrBlock(fmap1, fmap2, num_levels=num_levels, radius=radius),
        upsample=upsample_flow, warp=Resample2d(), range_map=range_map, census=CensusLoss(max_distance=3),
        smooth=SmoothnessLoss(order=2, edge_weighting="exponential", alpha=150.0, eps=0.001))


# ------------------------------------------------------------------ inputs
def _cast(d, dtype, device):
    return {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in d.items()}


def _images(rng, N, H, W, shift):
    """Two frames of one smooth scene, the second displaced by ``shift`` pixels, plus 2 % noise each, clipped to [0, 1]."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, (N, 3, 2, 1, 1))

    def scene(dx, dy):
        s = 0.5 + 0.06 * np.sin(2 * np.pi * (xs + dx) / 180.0 + ph[:, :, 0]) * np.cos(2 * np.pi * (ys + dy) / 120.0 + ph[:, :, 1])
        return s + 0.03 * np.sin(2 * np.pi * ((xs + dx) + 2 * (ys + dy)) / 61.0 + ph[:, :, 0])

    im1 = np.clip(scene(0.0, 0.0) + 0.02 * rng.standard_normal((N, 3, H, W)), 0.0, 1.0)
    im2 = np.clip(scene(*shift) + 0.02 * rng.standard_normal((N, 3, H, W)), 0.0, 1.0)
    return im1.astype(np.float32).astype(np.float64), im2.astype(np.float32).astype(np.float64)


RAFT_SHAPE = (2, 168, 224)          # maps 21 x 28 at stride 8; pyramid 21 x 28, 10 x 14, 5 x 7, 2 x 3
RAFT_CHANNELS, RAFT_HIDDEN, RAFT_LEVELS, RAFT_RADIUS, RAFT_ITERS = 32, 32, 4, 4, 3


def raft_inputs(seed=0, shape=RAFT_SHAPE):
    """{name: float64 array} of mini-RAFT: the two frames, the target flow and the parameters, every value a float32 number (so
    every dtype starts from the same numbers)."""
    N, H, W = shape
    rng = np.random.default_rng(seed)
    im1, im2 = _images(rng, N, H, W, (3.0, -2.0))
    C, Hd = RAFT_CHANNELS, RAFT_HIDDEN
    nc = RAFT_LEVELS * (2 * RAFT_RADIUS + 1) ** 2 + 2
    d = dict(im1=im1, im2=im2, target=SR._box9(8.0 * rng.standard_normal((N, 2, H, W))) * 4.0)
    d["fnet.weight"] = rng.standard_normal((C, 3, 8, 8)) * (12.0 / np.sqrt(3 * 64))
    d["fnet.bias"] = 0.1 * rng.standard_normal(C)
    d["update.weight"] = rng.standard_normal((Hd, nc, 3, 3)) / np.sqrt(nc * 9)
    d["update.bias"] = 0.1 * rng.standard_normal(Hd)
    d["delta.weight"] = rng.standard_normal((2, Hd, 3, 3)) * (1.5 / np.sqrt(Hd * 9 * 0.4))
    d["delta.bias"] = np.array([0.37, -0.21])
    d["mask.weight"] = rng.standard_normal((9 * 64, Hd, 1, 1)) * (4.0 / np.sqrt(Hd))
    d["mask.bias"] = 0.1 * rng.standard_normal(9 * 64)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in d.items()}


RAFT_PARAMS = ("fnet.weight", "fnet.bias", "update.weight", "update.bias", "delta.weight", "delta.bias", "mask.weight", "mask.bias")

UNSUP_SHAPE = (2, 36, 132)          # two tiles and four pixels both ways against 16 x 64; quarter resolution 9 x 33
MARGIN = 1.0 / 32


def unsup_inputs(seed=0, shape=UNSUP_SHAPE):
    """{name: float64 array} of the unsupervised loss: im1, im2, flow12 and flow21, every value a float32 number.
    flow12 is a 9 x 9 box-smoothed N(0, 6^2) field nudged so that every sample coordinate is at least 1/32 from an integer
    (the warp's flow gradient jumps at integers: a float32 and a float64 floor must agree); flow21 = rint(-2 flow12) / 2, so
    every splat weight is a multiple of 1/4 and the range map is exact in float32 under any summation order."""
    N, H, W = shape
    rng = np.random.default_rng(seed)
    im1, im2 = _images(rng, N, H, W, (2.5, -1.5))
    flow = SR._box9(6.0 * rng.standard_normal((N, 2, H, W))).astype(np.float32).astype(np.float64)
    frac = flow - np.rint(flow)                     # x and y are integers: the sample coordinate's distance to one
    near = np.abs(frac) < 2 * MARGIN
    flow = np.where(near, np.rint(flow) + np.where(frac < 0, -2 * MARGIN, 2 * MARGIN), flow).astype(np.float32).astype(np.float64)
    flow21 = np.rint(-2.0 * flow) / 2.0
    return dict(im1=im1, im2=im2, flow12=flow, flow21=flow21)


def check_unsup_inputs(inp):
    """The conditions of the unsupervised recipe's inputs, asserted by every test on its own data; returns the samples outside the image."""
    N, H, W = inp["flow12"].shape[0], *inp["flow12"].shape[2:]
    for k in ("im1", "im2"):
        assert inp[k].min() >= 0.0 and inp[k].max() <= 1.0 and inp[k].std() > 0.02
    f32 = inp["flow12"].astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), inp["flow12"])
    for dtype in (np.float32, np.float64):      # the coordinate as each precision forms it
        xf = np.arange(W, dtype=dtype)[None, None, :] + f32[:, 0].astype(dtype)
        yf = np.arange(H, dtype=dtype)[None, :, None] + f32[:, 1].astype(dtype)
        for c in (xf, yf):
            assert np.abs(c - np.rint(c)).min() >= MARGIN
    outside = (xf < 0) | (xf > W - 1) | (yf < 0) | (yf > H - 1)
    assert outside.mean() >= 0.01, outside.mean()
    assert np.array_equal(np.rint(2 * inp["flow21"]), 2 * inp["flow21"])
    return outside


# ------------------------------------------------------------------ mini-RAFT
def mini_raft(layers, t, mutation=None, upsample_input=None, context=contextlib.nullcontext):
    """One training step's forward and backward of a RAFT reduced to its wiring.  ``t``: the tensors of ``raft_inputs`` (the
    parameters get .grad).  Returns {flow_up_0 .. 2, loss, fmap1.grad, fmap2.grad, <parameter>.grad}.
    ``upsample_input`` maps the flow before ``upsample_flow`` (``.float()`` under autocast); the forward runs
    inside ``context()``, the backward outside it."""
    params = {k: t[k].detach().clone().requires_grad_(True) for k in RAFT_PARAMS}
    with context():
        im1, im2, target = t["im1"], t["im2"], t["target"]
        fmap1 = F.conv2d(im1 - 0.5, params["fnet.weight"], params["fnet.bias"], stride=8)
        fmap2 = F.conv2d(im2 - 0.5, params["fnet.weight"], params["fnet.bias"], stride=8)
        fmap1.retain_grad()
        fmap2.retain_grad()
        N, _, H, W = fmap1.shape
        corr_fn = layers.corr_block(fmap1, fmap2, RAFT_LEVELS, RAFT_RADIUS)
        ys, xs = torch.meshgrid(torch.arange(H, device=im1.device, dtype=im1.dtype), torch.arange(W, device=im1.device, dtype=im1.dtype),
                                indexing="ij")
        coords0 = torch.stack([xs, ys])[None].expand(N, 2, H, W).contiguous()
        coords1 = coords0.clone()
        flows = []
        for _ in range(RAFT_ITERS):
            if mutation != "coords_not_detached":
                coords1 = coords1.detach()
            corr = corr_fn(coords1)
            flow = coords1 - coords0
            h = torch.tanh(F.conv2d(torch.cat([corr, flow], 1), params["update.weight"], params["update.bias"], padding=1))
            coords1 = coords1 + F.conv2d(h, params["delta.weight"], params["delta.bias"], padding=1)
            up_mask = 0.25 * F.conv2d(h, params["mask.weight"], params["mask.bias"])
            flow = coords1 - coords0
            flows.append(layers.upsample(upsample_input(flow) if upsample_input else flow, up_mask))
        loss = sum(0.8 ** (RAFT_ITERS - 1 - i) * (f - target).abs().mean() for i, f in enumerate(flows))
    loss.backward()
    out = {"flow_up_%d" % i: f.detach() for i, f in enumerate(flows)}
    out.update({"loss": loss.detach(), "fmap1.grad": fmap1.grad, "fmap2.grad": fmap2.grad})
    out.update({k + ".grad": p.grad for k, p in params.items()})
    return out


# ------------------------------------------------------------------ the unsupervised loss
def unsup_loss(layers, t, mutation=None):
    """The UFlow-style loss of INTEGRATION.md, forward and backward.  ``t``: the tensors of ``unsup_inputs``.
    Returns {loss, photometric, smooth, noc, im1.grad, im2.grad, flow12.grad}."""
    im1, im2, flow12 = (t[k].detach().clone().requires_grad_(True) for k in ("im1", "im2", "flow12"))
    flow21 = t["flow21"]
    warp_flow = flow12.flip(1) if mutation == "flow_channels_swapped" else flow12
    im2_warped = layers.warp(im1 if mutation == "im1_warped" else im2, warp_flow.contiguous())
    noc = (layers.range_map(flow21) > 0.5).to(im1.dtype)
    photometric = layers.census(im1, im2_warped, 1 - noc if mutation == "noc_inverted" else noc)
    flow12_quarter = 0.25 * F.avg_pool2d(flow12, 4)
    im1_quarter = F.avg_pool2d(im1, 4)
    if mutation == "full_resolution_image_cropped":
        im1_quarter = im1[:, :, :im1_quarter.shape[2], :im1_quarter.shape[3]].contiguous()
    smooth = layers.smooth(flow12_quarter, im1_quarter.detach())
    loss = photometric + 4.0 * smooth
    loss.backward()
    return {"loss": loss.detach(), "photometric": photometric.detach(), "smooth": smooth.detach(), "noc": noc.detach(),
            "im1.grad": im1.grad, "im2.grad": torch.zeros_like(im2) if im2.grad is None else im2.grad, "flow12.grad": flow12.grad}


def run(pipeline, inputs, dtype, device="cpu", layers=None, **kw):
    return pipeline(layers or torch_layers(kw.get("mutation")), _cast(inputs, dtype, device), **kw)
