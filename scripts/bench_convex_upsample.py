"""ConvexUpsample (B = 8, C = 2): the fused layer against what a user writes without it -- RAFT's softmax / unfold / sum /
permute composition -- and against its own byte floor, in ONE process: machines differ by up to 20 %, so a number from another
run is not a baseline.

Rows: f = 8 at 48 x 64 and 55 x 128 (Sintel at 1/8) with float32 and float16 masks, f = 4 at 96 x 128 (float32).  Per row:
forward and backward (grad_mask + T, then the grad_flow gather) of the layer through the C ABI on preallocated tensors, and the
composition's forward and forward + backward through autograd, HIP events around windows of K calls, the contestants
alternating window by window, median / min / max window as microseconds per call; the algorithmic bytes of each direction
(every tensor read or written once; the backward also writes and reads T), their floor at the copy rate measured in this
process (float4 grid-stride copy of 1 GiB, read + write), and the share of that floor the kernels reach; the peak memory above
the inputs of forward + backward for the layer and for the composition.

    python scripts/bench_convex_upsample.py [--out profiles/convex_upsample_micro.json] [--windows 7] [--calls 10] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import fn2_capi  # noqa: E402
from bench_corr_dense import copy_ceiling, windows  # noqa: E402
from convex_upsample_ref import compose  # noqa: E402

B, C = 8, 2
ROWS = [(8, 48, 64, torch.float32), (8, 48, 64, torch.float16), (8, 55, 128, torch.float32), (8, 55, 128, torch.float16),
        (4, 96, 128, torch.float32)]


def algorithmic_bytes(f, H, W, msize):
    """(forward, backward) bytes: each tensor once; the backward re-reads flow and the mask, reads grad_out, writes grad_mask
    and grad_flow, and writes and reads the 9 C planes of T."""
    flow, mask, out, T = 4 * B * C * H * W, msize * B * 9 * f * f * H * W, 4 * B * C * f * f * H * W, 4 * B * C * 9 * H * W
    return flow + mask + out, flow + mask + out + mask + 2 * T + flow


def peak_above_inputs(fn, dev):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)


def row(f, H, W, dt, dev, gen, ceiling, n_windows, calls):
    from networks.upsample_package import ConvexUpsample
    flow = (10 * torch.randn(B, C, H, W, generator=gen)).to(dev)
    mask = (3 * torch.randn(B, 9 * f * f, H, W, generator=gen)).to(dt).to(dev)
    go = torch.randn(B, C, f * H, f * W, generator=gen).to(dev)
    scale = float(f)
    out = torch.empty(B, C, f * H, f * W, device=dev)
    grads = (torch.empty_like(flow), torch.empty_like(mask))
    ws = torch.empty(fn2_capi.upsample_lib().fn2u_convex_upsample_backward_workspace_bytes(B, C, H, W) // 4, device=dev)
    # the two must be the same function before their times mean anything
    with torch.no_grad():
        ref = compose(flow, mask.float(), f, scale)
        got = fn2_capi.convex_upsample_forward(flow, mask, f, scale)
        assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), "layer and composition differ"
    a, m = flow.clone().requires_grad_(True), mask.clone().requires_grad_(True)
    layer = ConvexUpsample(f)

    def comp_fb():
        a.grad = m.grad = None
        compose(a, m, f, scale).backward(go)

    def layer_fb():
        a.grad = m.grad = None
        layer(a, m).backward(go)

    with torch.no_grad():
        res = windows({"forward": lambda: fn2_capi.convex_upsample_forward(flow, mask, f, scale, out=out),
                       "composition_forward": lambda: compose(flow, mask, f, scale)}, n_windows, calls)
    res.update(windows({"backward": lambda: fn2_capi.convex_upsample_backward(flow, mask, go, f, scale, out=grads, workspace=ws),
                        "layer_forward_backward": layer_fb, "composition_forward_backward": comp_fb}, n_windows, calls))
    bf, bb = algorithmic_bytes(f, H, W, mask.element_size())
    for part, nbytes in (("forward", bf), ("backward", bb)):
        t = res[part]["median_us"] * 1e-6
        res[part].update({"algorithmic_MB": round(nbytes / 1e6, 1), "floor_us": round(nbytes / (ceiling * 1e9) * 1e6, 1),
                          "GBps": round(nbytes / t / 1e9, 1), "share_of_copy_ceiling": round(nbytes / t / 1e9 / ceiling, 3)})
    res["composition_over_layer_forward"] = round(res["composition_forward"]["median_us"] / res["forward"]["median_us"], 2)
    res["composition_over_layer_forward_backward"] = round(res["composition_forward_backward"]["median_us"] / res["layer_forward_backward"]["median_us"], 2)
    res["layer_peak_MB_above_inputs"] = peak_above_inputs(layer_fb, dev)
    res["composition_peak_MB_above_inputs"] = peak_above_inputs(comp_fb, dev)
    a.grad = m.grad = None
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
    gen = torch.Generator().manual_seed(0)
    ceiling = copy_ceiling(dev)
    torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "channels": C, "windows": a.windows, "calls_per_window": a.calls,
           "unit": "microseconds per call", "copy_ceiling_GBps": round(ceiling, 1), "rows": {}}
    for f, H, W, dt in (ROWS[:1] if a.quick else ROWS):
        name = f"f{f}_{H}x{W}_{str(dt).split('.')[-1]}"
        r = row(f, H, W, dt, dev, gen, ceiling, a.windows, a.calls)
        res["rows"][name] = r
        print(f"{name:22s} fwd {r['forward']['median_us']:8.1f} us ({r['forward']['share_of_copy_ceiling']:.2f} of the copy rate), composition "
              f"{r['composition_forward']['median_us']:8.1f} us | bwd {r['backward']['median_us']:8.1f} us ({r['backward']['share_of_copy_ceiling']:.2f}) | "
              f"fwd + bwd layer {r['layer_forward_backward']['median_us']:8.1f} composition {r['composition_forward_backward']['median_us']:8.1f} us | "
              f"peak {r['layer_peak_MB_above_inputs']} / {r['composition_peak_MB_above_inputs']} MB", file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
