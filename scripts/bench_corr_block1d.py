"""CorrBlock1D (staging; r = 4, L = 4, B = 8, C = 256, float32): the fused lookup of a prebuilt 1-D correlation pyramid against what
RAFT-Stereo's ``CorrBlock1D`` runs per iteration without it -- per level linspace, add, zeros_like, cat, grid_sample, view; then cat,
permute, contiguous -- on the SAME pyramid, in ONE process (machines differ by up to 20 %, so a number from another run is not a
baseline).

Maps 80 x 180 (a 320 x 720 crop at 1/4) and 94 x 311 (KITTI at 1/4), W2 = W1; coordinates = a smooth disparity, and uniform random.
Per row: forward per lookup and backward per lookup (the gradients of the four levels from grad_out), layer / composition, plus the
raw entry points into preallocated outputs ("kernel": no allocation, no autograd), HIP events around windows of K calls, the
contestants alternating window by window, median / min / max window as microseconds per call.  Per map: the build (einsum + pooling,
once per image pair), peak memory above the inputs of build + lookup + backward for the layer and for the composition, and both
kernels' bytes (windows read + output written; grad_out read + gradient levels written) over their time as a fraction of the copy
rate (read + write bytes per second of a 256 MiB device copy) measured here.

    python scripts/bench_corr_block1d.py [--out profiles/corr_block1d_micro.json] [--windows 7] [--calls 10] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_corr_block import copy_rate, peak_above_inputs  # noqa: E402
from bench_corr_dense import windows  # noqa: E402

B, C, R, LEVELS = 8, 256, 4, 4
MAPS = [(80, 180), (94, 311)]
D = 2 * R + 1


def composition_lookup(pyramid, coords):
    """RAFT-Stereo's CorrBlock1D.__call__ (core/corr.py, "reg") on a prebuilt pyramid."""
    cx = coords[:, :1].permute(0, 2, 3, 1)
    Bn, H, W, _ = cx.shape
    outs = []
    for lvl, corr in enumerate(pyramid):
        dx = torch.linspace(-R, R, D, dtype=cx.dtype, device=cx.device).view(D, 1)
        x0 = dx + cx.reshape(Bn * H * W, 1, 1, 1) / 2 ** lvl
        y0 = torch.zeros_like(x0)
        grid = torch.cat([2 * x0 / (corr.shape[-1] - 1) - 1, y0], dim=-1)
        outs.append(F.grid_sample(corr, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(Bn, H, W, -1))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous().float()


def composition_block(f1, f2, **_):
    """The composition's build, for the peak-memory row."""
    corr = torch.einsum("aijk,aijh->ajkh", f1, f2).reshape(-1, 1, 1, f2.shape[3]) / float(f1.shape[1]) ** 0.5
    pyr = [corr]
    for _ in range(LEVELS - 1):
        pyr.append(F.avg_pool2d(pyr[-1], [1, 2], stride=[1, 2]))
    return lambda co: composition_lookup(pyr, co)


def smooth_disparity(H, W, dev, gen):
    """B x 2 x H x W: x - d(x, y) with a smooth disparity d of 0 .. 0.3 W cells; channel 1 = y, as RAFT-Stereo keeps it."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ph = torch.rand(B, 1, 1, generator=gen) * 6.28
    d = 0.15 * W * (1 + torch.sin(0.021 * xs[None] + 0.033 * ys[None] + ph))
    return torch.stack([xs[None] - d, ys[None].expand(B, H, W)], 1).contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="the 80 x 180 map only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import fn2_capi
    from networks.correlation_package import CorrBlock1D, corr_sample1d
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    rate = copy_rate(dev)
    res = {"batch": B, "channels": C, "radius": R, "levels": LEVELS, "windows": a.windows,
           "calls_per_window": a.calls, "unit": "microseconds per call", "copy_rate_GBps": round(rate / 1e9, 1), "rows": {}, "maps": {}}
    for (H, W) in (MAPS[:1] if a.quick else MAPS):
        f1 = torch.randn(B, C, H, W, generator=gen).to(dev)
        f2 = torch.randn(B, C, H, W, generator=gen).to(dev)
        go = torch.randn(B, LEVELS * D, H, W, generator=gen).to(dev)
        with torch.no_grad():
            block = CorrBlock1D(f1, f2, num_levels=LEVELS, radius=R)
            build = windows({"build": lambda: CorrBlock1D(f1, f2, num_levels=LEVELS, radius=R)}, 3, 2, warm=1)["build"]
        pyramid = block.corr_pyramid
        cells = sum(t.numel() for t in pyramid)
        fwd_bytes = 4 * (LEVELS * B * H * W * (D + 1) + go.numel())
        bwd_bytes = 4 * (go.numel() + cells)
        rnd = torch.stack([torch.rand(B, H, W, generator=gen) * W, torch.zeros(B, H, W)], 1).to(dev)
        out_buf, grad_bufs = torch.empty_like(go), [torch.empty_like(t) for t in pyramid]
        for kind, co in (("smooth", smooth_disparity(H, W, dev, gen)), ("random", rnd)):
            with torch.no_grad():
                ref, out = composition_lookup(pyramid, co), block(co)
                assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), "the layer and the composition differ"
                fwd = windows({"layer": lambda: block(co), "composition": lambda: composition_lookup(pyramid, co),
                               "kernel": lambda: fn2_capi.corr_sample1d_forward(pyramid, co, R, out=out_buf)}, a.windows, a.calls)
            leaves = [t.clone().requires_grad_(True) for t in pyramid]
            ours, theirs = corr_sample1d(leaves, co, R), composition_lookup(leaves, co)
            bwd = windows({"layer": lambda: torch.autograd.grad(ours, leaves, go, retain_graph=True),
                           "composition": lambda: torch.autograd.grad(theirs, leaves, go, retain_graph=True),
                           "kernel": lambda: fn2_capi.corr_sample1d_backward(pyramid, co, go, R, out=grad_bufs)}, a.windows, a.calls)
            del leaves, ours, theirs
            row = {"forward": fwd, "backward": bwd}
            for part, nbytes in (("forward", fwd_bytes), ("backward", bwd_bytes)):
                row[part]["composition_over_layer_median"] = round(row[part]["composition"]["median_us"] / row[part]["layer"]["median_us"], 2)
                row[part]["kernel_MB"] = round(nbytes / 1e6, 1)
                row[part]["kernel_fraction_of_copy_rate"] = round(nbytes / (row[part]["kernel"]["median_us"] * 1e-6) / rate, 3)
            res["rows"][f"{H}x{W}_{kind}"] = row
            print(f"{H}x{W} {kind}: {row}", file=sys.stderr, flush=True)
        co = smooth_disparity(H, W, dev, gen)
        del out_buf, grad_bufs

        def step(make):
            a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
            make(a1, a2, num_levels=LEVELS, radius=R)(co).backward(go)

        m = {"build": build, "pyramid_MB": round(4 * cells / 1e6, 1),
             "corr_block1d_peak_MB_above_inputs": peak_above_inputs(lambda: step(CorrBlock1D), dev),
             "composition_peak_MB_above_inputs": peak_above_inputs(lambda: step(composition_block), dev)}
        res["maps"][f"{H}x{W}"] = m
        print(f"{H}x{W}: {m}", file=sys.stderr, flush=True)
        del block, pyramid
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
