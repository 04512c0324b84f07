"""The structural-similarity distance (float32): the layer against what a user writes without it -- five ``avg_pool2d`` over x, y,
x^2, y^2, xy and the elementwise quotient and clamp, tests/ssim_ref.compose -- and against the chip's copy rate, in ONE process:
machines differ by up to 20 %, so a number from another run is not a baseline.

Rows: 8 x 3 x 384 x 512 (full resolution) and 8 x 3 x 96 x 128 (quarter resolution), md 1 and 3, both borders; inputs: the noise
family of the tests.  Per row: the forward and the backward kernel (both gradients, and im2's alone, the one a warped second frame
needs) through the C ABI on preallocated tensors, the composition's forward, and forward + backward through autograd for the layer
and for the composition; HIP events around windows of K calls after a warm-up window, the contestants alternating window by
window, median / min / max window as microseconds per call; the peak memory above the inputs of both; the bytes the operation has
to move (two images in, one out; the backward three in, two out) with the time they take at the copy rate measured in this process.

    python scripts/ssim_micro.py [--out profiles/ssim_micro.json] [--windows 7] [--calls 10] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import fn2_capi  # noqa: E402
import ssim_ref as R  # noqa: E402
from bench_census import peak_above_inputs  # noqa: E402
from bench_corr_dense import copy_ceiling, windows  # noqa: E402

ROWS = [(shape, md, border) for shape in ((8, 3, 384, 512), (8, 3, 96, 128)) for md in (1, 3) for border in ("zero", "reflect")]


def row(shape, md, border, dev, ceiling, n_windows, calls):
    from networks.ssim_package import SSIM
    im1, im2, go = (t.float().to(dev) for t in R.inputs(shape, "noise", seed=17))
    out, g1, g2 = torch.empty_like(im1), torch.empty_like(im1), torch.empty_like(im2)
    layer = SSIM(md, R.C1, R.C2, border)
    # the two must be the same function before their times mean anything
    a, b = im1.clone().requires_grad_(True), im2.clone().requires_grad_(True)
    ref = R.compose(a, b, md, R.C1, R.C2, border)
    ref.backward(go)
    ca, cb = a.grad.clone(), b.grad.clone()
    a.grad = b.grad = None
    got = layer(a, b)
    got.backward(go)
    assert float((got - ref).detach().abs().max()) <= 1e-4, "layer and composition differ"
    for g, want in ((a.grad, ca), (b.grad, cb)):
        assert float((g - want).abs().max()) <= 1e-3 * float(want.abs().max()), "layer and composition gradients differ"

    def comp_fb():
        a.grad = b.grad = None
        R.compose(a, b, md, R.C1, R.C2, border).backward(go)

    def layer_fb():
        a.grad = b.grad = None
        layer(a, b).backward(go)

    with torch.no_grad():
        res = windows({"forward": lambda: fn2_capi.ssim_forward(im1, im2, md, R.C1, R.C2, border, out=out),
                       "backward": lambda: fn2_capi.ssim_backward(im1, im2, go, md, R.C1, R.C2, border, grads=(g1, g2)),
                       "backward_im2_only": lambda: fn2_capi.ssim_backward(im1, im2, go, md, R.C1, R.C2, border, want1=False, grads=(None, g2)),
                       "composition_forward": lambda: R.compose(im1, im2, md, R.C1, R.C2, border)}, n_windows, calls)
    res.update(windows({"layer_forward_backward": layer_fb, "composition_forward_backward": comp_fb}, n_windows, calls))
    nbytes = 4 * im1.numel()
    for part, moved in (("forward", 3 * nbytes), ("backward", 5 * nbytes)):
        floor = moved / (ceiling * 1e9) * 1e6
        res[part].update({"algorithmic_MB": round(moved / 1e6, 1), "copy_floor_us": round(floor, 1),
                          "share_of_copy_ceiling": round(floor / res[part]["median_us"], 3)})
    res["input_MB"] = round(2 * nbytes / 1e6, 1)
    res["composition_over_layer_forward"] = round(res["composition_forward"]["median_us"] / res["forward"]["median_us"], 2)
    res["composition_over_layer_forward_backward"] = round(res["composition_forward_backward"]["median_us"] /
                                                           res["layer_forward_backward"]["median_us"], 2)
    res["layer_peak_MB_above_inputs"] = peak_above_inputs(layer_fb, dev)
    res["composition_peak_MB_above_inputs"] = peak_above_inputs(comp_fb, dev)
    a.grad = b.grad = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="the first row only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    ceiling = copy_ceiling(dev)
    torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "windows": a.windows, "calls_per_window": a.calls, "unit": "microseconds per call",
           "copy_ceiling_GBps": round(ceiling, 1), "rows": {}}
    for shape, md, border in ROWS[:1 if a.quick else None]:
        name = "x".join(map(str, shape)) + f"_md{md}_{border}"
        r = row(shape, md, border, dev, ceiling, a.windows, a.calls)
        res["rows"][name] = r
        print(f"{name:30s} fwd {r['forward']['median_us']:8.1f} composition {r['composition_forward']['median_us']:9.1f} us | bwd "
              f"{r['backward']['median_us']:8.1f} (im2 only {r['backward_im2_only']['median_us']:8.1f}) us | fwd + bwd layer "
              f"{r['layer_forward_backward']['median_us']:8.1f} composition {r['composition_forward_backward']['median_us']:9.1f} us | copy floor fwd "
              f"{r['forward']['copy_floor_us']} bwd {r['backward']['copy_floor_us']} us | peak {r['layer_peak_MB_above_inputs']} / "
              f"{r['composition_peak_MB_above_inputs']} MB", file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
