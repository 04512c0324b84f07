"""CorrPyramid (incubating; L = 4, B = 8, C = 256, float32): the fused build of RAFT's all-pairs pyramid against what
``CorrBlock.__init__`` composes without it -- ``torch.matmul``, a division by sqrt(C), three ``avg_pool2d`` -- in ONE process
(machines differ by up to 20 %, so a number from another run is not a baseline).

Maps 48 x 64 and 55 x 128 (Sintel at 1/8).  Per map: build forward, and build forward + backward (from the gradients of all four
levels to the gradients of both maps), fused / composition, HIP events around windows of K calls, the contestants alternating window
by window, median / min / max window as microseconds per call; the three parts of the composition on their own (matmul, scale,
pooling); ``torch.cuda.max_memory_allocated`` above the inputs for both, forward and forward + backward; and the bytes the fused
forward writes (the pyramid) and the fold moves (gradient levels read + G written) over their time as a share of the store rate (bytes
per second of a 1 GiB fill) measured here.

    python scripts/bench_corr_pyramid.py [--out profiles/corr_pyramid_micro.json] [--windows 7] [--calls 5] [--quick]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_corr_block import peak_above_inputs  # noqa: E402
from bench_corr_dense import windows  # noqa: E402

B, C, LEVELS = 8, 256, 4
MAPS = [(48, 64), (55, 128)]


def composition(f1, f2):
    """CorrBlock.__init__ (networks/correlation_package/corr_block.py, RAFT's core/corr.py)."""
    Bn, Cn, H, W = f1.shape
    corr = torch.matmul(f1.reshape(Bn, Cn, H * W).transpose(1, 2), f2.reshape(Bn, Cn, -1)) / math.sqrt(Cn)
    pyr = [corr.reshape(Bn * H * W, 1, *f2.shape[2:])]
    for _ in range(LEVELS - 1):
        pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
    return pyr


def store_rate(dev):
    """Bytes per second of a 1 GiB fill: the best of five windows of four."""
    dst = torch.empty(1 << 28, device=dev)
    t = windows({"fill": lambda: dst.fill_(1.0)}, 5, 4)["fill"]["min_us"]
    return dst.numel() * 4 / (t * 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the 48 x 64 map only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import fn2_capi
    from networks.correlation_package.corr_pyramid import corr_pyramid
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    rate = store_rate(dev)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "channels": C, "levels": LEVELS, "windows": a.windows,
           "calls_per_window": a.calls, "unit": "microseconds per call", "store_rate_GBps": round(rate / 1e9, 1), "maps": {}}
    for (H, W) in (MAPS[:1] if a.quick else MAPS):
        f1 = torch.randn(B, C, H, W, generator=gen).to(dev)
        f2 = torch.randn(B, C, H, W, generator=gen).to(dev)
        M = H * W
        with torch.no_grad():
            ours, ref = corr_pyramid(f1, f2, LEVELS), composition(f1, f2)
            for x, y in zip(ours, ref):
                assert float((x - y).abs().max()) <= 1e-4 * float(y.abs().max()), "the layer and the composition differ"
            cells = sum(t.numel() for t in ours)
            del ours, ref
            fwd = windows({"fused": lambda: corr_pyramid(f1, f2, LEVELS), "composition": lambda: composition(f1, f2)}, a.windows, a.calls)
            # the composition's parts
            A, Bm = f1.reshape(B, C, M).transpose(1, 2), f2.reshape(B, C, M)
            raw = torch.matmul(A, Bm)
            vol = (raw / math.sqrt(C)).reshape(B * M, 1, H, W)

            def pooling():
                x = vol
                for _ in range(LEVELS - 1):
                    x = F.avg_pool2d(x, 2, stride=2)

            parts = windows({"matmul": lambda: torch.matmul(A, Bm), "scale": lambda: raw / math.sqrt(C), "pooling": pooling}, a.windows, a.calls)
            del raw, vol
        gouts = [torch.randn(B * M, 1, H >> l, W >> l, device=dev) for l in range(LEVELS)]
        a1, a2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)

        def train(build):
            torch.autograd.backward(build(a1, a2), gouts)
            a1.grad = a2.grad = None

        both = windows({"fused": lambda: train(lambda x, y: corr_pyramid(x, y, LEVELS)), "composition": lambda: train(composition)},
                       a.windows, a.calls)
        G = torch.empty(B * M, H, W, device=dev)
        fold = windows({"fold": lambda: fn2_capi.corr_pyramid_fold(gouts, (B, C, H, W, H, W), out=G)}, a.windows, a.calls)["fold"]
        del G
        with torch.no_grad():
            peak_f = {"fused": peak_above_inputs(lambda: corr_pyramid(f1, f2, LEVELS), dev), "composition": peak_above_inputs(lambda: composition(f1, f2), dev)}
        peak_b = {"fused": peak_above_inputs(lambda: train(lambda x, y: corr_pyramid(x, y, LEVELS)), dev),
                  "composition": peak_above_inputs(lambda: train(composition), dev)}
        tf = fwd["fused"]["median_us"]
        m = {"forward": fwd, "forward_backward": both, "composition_parts": parts, "fold": fold,
             "composition_over_fused_forward": round(fwd["composition"]["median_us"] / tf, 2),
             "composition_over_fused_forward_backward": round(both["composition"]["median_us"] / both["fused"]["median_us"], 2),
             "pyramid_MB": round(4 * cells / 1e6, 1),
             "forward_share_of_store_rate": round(4 * cells / (tf * 1e-6) / rate, 3),
             "fold_MB": round(4 * (cells + B * M * M) / 1e6, 1),
             "fold_share_of_store_rate": round(4 * (cells + B * M * M) / (fold["median_us"] * 1e-6) / rate, 3),
             "mfma_TFLOPs_bf16": round(6 * 2 * B * M * M * C / (tf * 1e-6) / 1e12, 1),
             "forward_peak_MB_above_inputs": peak_f, "forward_backward_peak_MB_above_inputs_and_grad_levels": peak_b}
        res["maps"][f"{H}x{W}"] = m
        print(f"{H}x{W}: {m}", file=sys.stderr, flush=True)
        del gouts, a1, a2
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
