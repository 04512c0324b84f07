"""The edge-aware smoothness term (float32): the layer against what a user writes without it -- image gradients, abs or square, the
channel mean, exp, flow gradients taken once or twice, the robust function, the products and the zero padding, about twenty
elementwise launches -- and against the chip's copy rate, each row in ONE process: machines differ by up to 20 %, so a number from
another run is not a baseline.

Rows: 8 x 2 x 384 x 512 with a 3-channel image, and 8 x 2 x 96 x 128, the quarter-resolution level where UFlow applies the term; both
orders and both edge weightings.  Per row: the forward and the backward through the C ABI on preallocated tensors, the
composition's forward and forward + backward through autograd and the layer's forward + backward, HIP events around windows of K
calls, the contestants alternating window by window, median / min / max window as microseconds per call; the peak memory above the
inputs of both; and the bytes each kernel has to move (flow and image in, two planes out; the backward flow, image and grad_out
in, the flow gradient out) with the time they take at the copy rate measured in the same process.

The driver runs every row as a child process of its own under a time limit and stops at the first one that fails or runs out of
time; nothing is started on the GPU after a failure.

    python scripts/bench_smoothness.py [--out profiles/smoothness_micro.json] [--windows 7] [--calls 50] [--quick]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

SHAPES = [(8, 2, 3, 384, 512), (8, 2, 3, 96, 128)]   # N, F, C, H, W
ROWS = [(s, k, e) for s in SHAPES for k in (1, 2) for e in ("exponential", "gaussian")]
ALPHA, EPS = 150.0, 0.001   # on smoothness_ref's first image family: alpha 150 on a 5 % image
ROW_TIMEOUT_S = 240


def row_name(shape, order, edge):
    return "x".join(map(str, shape)) + f"_order{order}_{edge}"


def peak_above_inputs(fn, dev):
    import torch
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 2)


def row(shape, order, edge, n_windows, calls):
    """One row, measured in this process: the copy rate first, then the layer and the composition alternating."""
    import torch

    import fn2_capi
    import smoothness_ref as RS
    from bench_corr_dense import copy_ceiling, windows
    from networks.smoothness_package import EdgeAwareSmoothness
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    ceiling = copy_ceiling(dev)
    torch.cuda.empty_cache()
    N, F, C, H, W = shape
    flow, image, go, _ = (torch.from_numpy(a).to(dev) if hasattr(a, "shape") else a for a in RS.inputs(shape, 0, 17))
    out = torch.empty(N, 2, H, W, device=dev)
    gflow = torch.empty_like(flow)
    args = (order, edge, ALPHA, EPS)
    # the two must be the same function before their times mean anything
    x = flow.clone().requires_grad_(True)
    ref = RS.compose(x, image, *args)
    ref.backward(go)
    got = fn2_capi.smoothness_forward(flow, image, *args)
    assert float((got - ref.detach()).abs().max()) <= 1e-4 * float(ref.detach().abs().max()), "layer and composition differ"
    cg = x.grad.clone()
    lg = fn2_capi.smoothness_backward(flow, image, go, *args)
    assert float((lg - cg).abs().max()) <= 1e-4 * float(cg.abs().max()), "layer and composition gradients differ"
    layer = EdgeAwareSmoothness(*args)

    def comp_fb():
        x.grad = None
        RS.compose(x, image, *args).backward(go)

    def layer_fb():
        x.grad = None
        layer(x, image).backward(go)

    with torch.no_grad():
        res = windows({"forward": lambda: fn2_capi.smoothness_forward(flow, image, *args, out=out),
                       "backward": lambda: fn2_capi.smoothness_backward(flow, image, go, *args, out=gflow),
                       "composition_forward": lambda: RS.compose(flow, image, *args)}, n_windows, calls)
    res.update(windows({"layer_forward_backward": layer_fb, "composition_forward_backward": comp_fb}, n_windows, calls))
    plane = 4 * N * H * W
    moved = {"forward": (F + C + 2) * plane, "backward": (F + C + 2 + F) * plane}
    for part, nbytes in moved.items():
        t = res[part]["median_us"]
        floor = nbytes / (ceiling * 1e9) * 1e6
        res[part].update({"algorithmic_MB": round(nbytes / 1e6, 2), "copy_floor_us": round(floor, 2), "share_of_copy_ceiling": round(floor / t, 3)})
    res["input_MB"] = round((F + C) * plane / 1e6, 2)
    res["composition_over_layer_forward"] = round(res["composition_forward"]["median_us"] / res["forward"]["median_us"], 2)
    res["composition_over_layer_forward_backward"] = round(res["composition_forward_backward"]["median_us"] /
                                                           res["layer_forward_backward"]["median_us"], 2)
    res["layer_peak_MB_above_inputs"] = peak_above_inputs(layer_fb, dev)
    res["composition_peak_MB_above_inputs"] = peak_above_inputs(comp_fb, dev)
    with torch.no_grad():
        res["composition_forward_peak_MB_above_inputs"] = peak_above_inputs(lambda: RS.compose(flow, image, *args), dev)
        res["layer_forward_peak_MB_above_inputs"] = peak_above_inputs(lambda: layer(flow, image), dev)
    props = torch.cuda.get_device_properties(dev)
    res["copy_ceiling_GBps"] = round(ceiling, 1)
    res["device"] = torch.cuda.get_device_name(0)
    res["compute_units"] = props.multi_processor_count
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="the first row only")
    ap.add_argument("--row", type=int, default=None, help="(child) measure this row in this process and print its JSON")
    a = ap.parse_args()
    if a.row is not None:
        print(json.dumps(row(*ROWS[a.row], a.windows, a.calls)))
        return 0
    res = {"windows": a.windows, "calls_per_window": a.calls, "unit": "microseconds per call", "alpha": ALPHA, "eps": EPS, "rows": {}}
    for i, (shape, order, edge) in enumerate(ROWS[:1 if a.quick else None]):
        name = row_name(shape, order, edge)
        cmd = [sys.executable, os.path.abspath(__file__), "--row", str(i), "--windows", str(a.windows), "--calls", str(a.calls)]
        try:
            pr = subprocess.run(cmd, capture_output=True, text=True, timeout=ROW_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result after {ROW_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 1
        if pr.returncode != 0:
            print(f"{name}: exit status {pr.returncode}; stopping\n{pr.stderr[-3000:]}", file=sys.stderr)
            return 1
        r = json.loads(pr.stdout.strip().splitlines()[-1])
        for key in ("device", "compute_units"):
            res[key] = r.pop(key)
        res["rows"][name] = r
        print(f"{name:44s} fwd {r['forward']['median_us']:7.1f} ({r['forward']['share_of_copy_ceiling']:.2f} of copy) composition "
              f"{r['composition_forward']['median_us']:8.1f} us | bwd {r['backward']['median_us']:7.1f} ({r['backward']['share_of_copy_ceiling']:.2f}) us | "
              f"fwd + bwd layer {r['layer_forward_backward']['median_us']:7.1f} composition {r['composition_forward_backward']['median_us']:8.1f} us | "
              f"peak {r['layer_peak_MB_above_inputs']} / {r['composition_peak_MB_above_inputs']} MB | copy {r['copy_ceiling_GBps']} GB/s",
              file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
