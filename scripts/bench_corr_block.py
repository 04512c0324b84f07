"""CorrBlock (preview; r = 4, L = 4, B = 8, C = 256, float32): the fused lookup of a prebuilt all-pairs pyramid against what RAFT's
``CorrBlock`` runs per iteration without it -- four ``grid_sample`` calls, cat, permute -- on the SAME pyramid, and against
``AlternateCorrBlock``, all in ONE process (machines differ by up to 20 %, so a number from another run is not a baseline).

Maps 48 x 64 and 55 x 128 (Sintel at 1/8); coordinates = identity + a smooth flow of up to 3 pixels, and uniform random.  Per row:
forward per lookup and backward per lookup (the gradients of the four levels from grad_out), layer / composition / AlternateCorrBlock,
HIP events around windows of K calls, the contestants alternating window by window, median / min / max window as microseconds per
call.  Per map: the build (matmul + pooling, once per image pair), peak memory above the inputs of build + lookup + backward for
CorrBlock and for AlternateCorrBlock, and both kernels' bytes (patches read + output written; grad_out read + gradient levels
written) over their time as a fraction of the copy rate (read + write bytes per second of a 256 MiB device copy) measured here.

    python scripts/bench_corr_block.py [--out profiles/corr_block_micro.json] [--windows 7] [--calls 10] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_corr_dense import windows  # noqa: E402
from bench_corr_lookup import smooth_coords  # noqa: E402

B, C, R, LEVELS = 8, 256, 4, 4
MAPS = [(48, 64), (55, 128)]
D = 2 * R + 1


def composition_lookup(pyramid, coords):
    """RAFT's CorrBlock.__call__ (core/corr.py) on a prebuilt pyramid."""
    Bn, _, H, W = coords.shape
    d = torch.linspace(-R, R, D, dtype=coords.dtype, device=coords.device)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, D, D, 2)
    centroid = coords.permute(0, 2, 3, 1).reshape(Bn * H * W, 1, 1, 2)
    outs = []
    for lvl, corr in enumerate(pyramid):
        h2, w2 = corr.shape[-2:]
        xy = centroid / 2 ** lvl + delta
        grid = torch.stack((2 * xy[..., 0] / (w2 - 1) - 1, 2 * xy[..., 1] / (h2 - 1) - 1), dim=-1)
        outs.append(F.grid_sample(corr, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(Bn, H, W, D * D))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def copy_rate(dev):
    """Bytes per second, read + write, of a 256 MiB device-to-device copy: the best of five windows of four."""
    src = torch.empty(1 << 26, device=dev)
    dst = torch.empty_like(src)
    t = windows({"copy": lambda: dst.copy_(src)}, 5, 4)["copy"]["min_us"]
    return 2 * src.numel() * 4 / (t * 1e-6)


def peak_above_inputs(fn, dev):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="the 48 x 64 map only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from networks.correlation_package import AlternateCorrBlock, CorrBlock, corr_sample
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    rate = copy_rate(dev)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "channels": C, "radius": R, "levels": LEVELS, "windows": a.windows,
           "calls_per_window": a.calls, "unit": "microseconds per call", "copy_rate_GBps": round(rate / 1e9, 1), "rows": {}, "maps": {}}
    for (H, W) in (MAPS[:1] if a.quick else MAPS):
        f1 = torch.randn(B, C, H, W, generator=gen).to(dev)
        f2 = torch.randn(B, C, H, W, generator=gen).to(dev)
        go = torch.randn(B, LEVELS * D * D, H, W, generator=gen).to(dev)
        with torch.no_grad():
            block = CorrBlock(f1, f2, num_levels=LEVELS, radius=R)
            alt = AlternateCorrBlock(f1, f2, num_levels=LEVELS, radius=R)
            build = windows({"build": lambda: CorrBlock(f1, f2, num_levels=LEVELS, radius=R)}, 3, 2, warm=1)["build"]
        cells = sum(t.numel() for t in block.corr_pyramid)
        fwd_bytes = 4 * (LEVELS * B * H * W * (D + 1) ** 2 + go.numel())
        bwd_bytes = 4 * (go.numel() + cells)
        rnd = torch.stack([torch.rand(B, H, W, generator=gen) * W, torch.rand(B, H, W, generator=gen) * H], 1).to(dev)
        for kind, co in (("smooth", smooth_coords(H, W, dev, gen)), ("random", rnd)):
            with torch.no_grad():
                ref, out = composition_lookup(block.corr_pyramid, co), block(co)
                assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), "the layer and the composition differ"
                fwd = windows({"layer": lambda: block(co), "composition": lambda: composition_lookup(block.corr_pyramid, co),
                               "alternate": lambda: alt(co)}, a.windows, a.calls)
            leaves = [t.clone().requires_grad_(True) for t in block.corr_pyramid]
            ours, theirs = corr_sample(leaves, co, R), composition_lookup(leaves, co)
            a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
            alts = AlternateCorrBlock(a1, a2, num_levels=LEVELS, radius=R)(co)
            bwd = windows({"layer": lambda: torch.autograd.grad(ours, leaves, go, retain_graph=True),
                           "composition": lambda: torch.autograd.grad(theirs, leaves, go, retain_graph=True)}, a.windows, a.calls)
            bwd.update(windows({"alternate": lambda: torch.autograd.grad(alts, (a1, a2), go, retain_graph=True)}, 3, 2, warm=1))
            del leaves, ours, theirs, alts
            row = {"forward": fwd, "backward": bwd}
            for part, nbytes in (("forward", fwd_bytes), ("backward", bwd_bytes)):
                t = row[part]["layer"]["median_us"]
                row[part]["composition_over_layer_median"] = round(row[part]["composition"]["median_us"] / t, 2)
                row[part]["alternate_over_layer_median"] = round(row[part]["alternate"]["median_us"] / t, 2)
                row[part]["layer_MB"] = round(nbytes / 1e6, 1)
                row[part]["layer_fraction_of_copy_rate"] = round(nbytes / (t * 1e-6) / rate, 3)
            res["rows"][f"{H}x{W}_{kind}"] = row
            print(f"{H}x{W} {kind}: {row}", file=sys.stderr, flush=True)
        co = smooth_coords(H, W, dev, gen)

        def step(make):
            a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
            make(a1, a2, num_levels=LEVELS, radius=R)(co).backward(go)

        m = {"build": build, "all_pairs_pyramid_MB": round(4 * cells / 1e6, 1),
             "corr_block_peak_MB_above_inputs": peak_above_inputs(lambda: step(CorrBlock), dev),
             "alternate_peak_MB_above_inputs": peak_above_inputs(lambda: step(AlternateCorrBlock), dev)}
        res["maps"][f"{H}x{W}"] = m
        print(f"{H}x{W}: {m}", file=sys.stderr, flush=True)
        del block, alt
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
