"""ForwardWarp (float32): the layer against what a user writes without it -- four ``index_put_(accumulate=True)`` over index
tensors -- and against the chip's float atomic rate, in ONE process: machines differ by up to 20 %, so a number from another run
is not a baseline.

Rows: 8 x 32 x 96 x 128 (features at 1/4 of Sintel) and 8 x 3 x 384 x 512 (images), each with the smooth and the random flow
family of the tests.  Per row: the general, tiled and deterministic forward and the backward through the C ABI on preallocated
tensors, the composition's forward and forward + backward through autograd and the layer's forward + backward, HIP events around
windows of K calls, the contestants alternating window by window, median / min / max window as microseconds per call; the
peak memory above the inputs of both; and the atomic bytes each forward adds per input byte, counted from the flow with the
kernels' rules, with the time those bytes take at 1.3 TB/s of added bytes (the chip-wide float atomic rate) next to the copy
rate measured in this process.  Last, a sweep of both forwards over flows of growing disorder at both shapes -- zero, half a
pixel everywhere (four contiguous taps), the smooth family with integer rows, the smooth family -- which separates what the global
atomics cost from what the tiled kernel costs whatever the flow.

    python scripts/bench_forward_warp.py [--out profiles/forward_warp_micro.json] [--windows 7] [--calls 10] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fn2_capi  # noqa: E402
import forward_warp_ref as RS  # noqa: E402
from bench_corr_dense import copy_ceiling, windows  # noqa: E402

ROWS = [(8, 32, 96, 128), (8, 3, 384, 512)]
FAMILIES = ["smooth", "random"]
ATOMIC_GBPS = 1300.0


def atomics_per_pixel(flow):
    """Global atomic adds per source pixel and channel: (general, tiled).  General: the taps inside the image of non-zero
    weight.  Tiled: per tile the patch cells inside the image that an in-patch pixel touches (an upper count: a cell whose sum
    is exactly zero is skipped), plus the general count of the pixels that leave the patch."""
    m = RS.header_macros()
    TH, TW, HALO = m["FN2S_TILE_H"], m["FN2S_TILE_W"], m["FN2S_HALO"]
    PH, PW = TH + 2 * HALO, TW + 2 * HALO
    B, _, H, W = flow.shape
    t = RS.taps(flow)
    ws = RS._weights(t, np.float32)
    per_pixel = np.zeros((B, H, W), np.int64)
    for (dy, dx), w in zip(RS.TAPS, ws):
        per_pixel += RS._inside(t, dy, dx, H, W)[0] & (w != 0)
    general = per_pixel.sum()
    tiled = 0
    for b in range(B):
        for Y0 in range(0, H, TH):
            for X0 in range(0, W, TW):
                cy, cx = min(Y0 + TH // 2, H - 1), min(X0 + TW // 2, W - 1)
                off = [int(np.rint(v)) if abs(v) < 1e6 else 0 for v in (flow[b, 0, cy, cx], flow[b, 1, cy, cx])]
                px0, py0 = X0 - HALO + off[0], Y0 - HALO + off[1]
                sl = (b, slice(Y0, Y0 + TH), slice(X0, X0 + TW))
                lx, ly = t["x0"][sl] - px0, t["y0"][sl] - py0
                inp = t["valid"][sl] & (lx >= 0) & (lx <= PW - 2) & (ly >= 0) & (ly <= PH - 2)
                tiled += per_pixel[sl][t["valid"][sl] & ~inp].sum()
                patch = np.zeros((PH, PW), bool)
                for dy, dx in RS.TAPS:
                    patch[ly[inp] + dy, lx[inp] + dx] = True
                ys, xs = np.nonzero(patch)
                tiled += ((ys + py0 >= 0) & (ys + py0 < H) & (xs + px0 >= 0) & (xs + px0 < W)).sum()
    return general / (B * H * W), tiled / (B * H * W)


def peak_above_inputs(fn, dev):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)


def row(shape, family, dev, gen, ceiling, n_windows, calls):
    from networks.splat_package import ForwardWarp
    B, C, H, W = shape
    x = torch.randn(shape, generator=gen).to(dev)
    go = torch.randn(shape, generator=gen).to(dev)
    flow_np = RS.flow_family(family, B, H, W)
    flow = torch.from_numpy(flow_np).to(dev)
    out = torch.empty_like(x)
    ws = torch.empty(fn2_capi.splat_lib().fn2s_forward_warp_forward_det_workspace_bytes(*shape) // 8, dtype=torch.int64, device=dev)
    # the two must be the same function before their times mean anything
    with torch.no_grad():
        ref = RS.compose(x, flow)
        for algo in (fn2_capi.FN2S_GENERAL, fn2_capi.FN2S_TILED):
            got = fn2_capi.forward_warp_forward(x, flow, algo)
            assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), "layer and composition differ"
        got = fn2_capi.forward_warp_forward_det(x, flow, workspace=ws)
        assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), "deterministic forward and composition differ"
    a, f = x.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    layer = ForwardWarp()

    def comp_fb():
        a.grad = f.grad = None
        RS.compose(a, f).backward(go)

    def layer_fb():
        a.grad = f.grad = None
        layer(a, f).backward(go)

    with torch.no_grad():
        res = windows({"forward_general": lambda: fn2_capi.forward_warp_forward(x, flow, fn2_capi.FN2S_GENERAL, out=out),
                       "forward_tiled": lambda: fn2_capi.forward_warp_forward(x, flow, fn2_capi.FN2S_TILED, out=out),
                       "forward_deterministic": lambda: fn2_capi.forward_warp_forward_det(x, flow, out=out, workspace=ws),
                       "backward": lambda: fn2_capi.forward_warp_backward(x, flow, go),
                       "composition_forward": lambda: RS.compose(x, flow)}, n_windows, calls)
    res.update(windows({"layer_forward_backward": layer_fb, "composition_forward_backward": comp_fb}, n_windows, calls))
    in_bytes = 4 * B * C * H * W
    per_g, per_t = atomics_per_pixel(flow_np)
    for part, per in (("forward_general", per_g), ("forward_tiled", per_t)):
        t = res[part]["median_us"] * 1e-6
        res[part].update({"atomic_bytes_per_input_byte": round(float(per), 3), "atomic_MB": round(per * in_bytes / 1e6, 1),
                          "atomic_floor_us": round(per * in_bytes / (ATOMIC_GBPS * 1e9) * 1e6, 1),
                          "atomic_GBps": round(per * in_bytes / t / 1e9, 1)})
    # the backward reads input, grad_out (four taps, counted once) and flow and writes both gradients
    bwd = 3 * in_bytes + 4 * 4 * B * H * W
    res["backward"].update({"algorithmic_MB": round(bwd / 1e6, 1), "floor_us": round(bwd / (ceiling * 1e9) * 1e6, 1),
                            "share_of_copy_ceiling": round(bwd / (res["backward"]["median_us"] * 1e-6) / 1e9 / ceiling, 3)})
    res["input_MB"] = round(in_bytes / 1e6, 1)
    res["tiled_over_general"] = round(res["forward_tiled"]["median_us"] / res["forward_general"]["median_us"], 3)
    res["composition_over_tiled_forward"] = round(res["composition_forward"]["median_us"] / res["forward_tiled"]["median_us"], 2)
    res["composition_over_layer_forward_backward"] = round(res["composition_forward_backward"]["median_us"] / res["layer_forward_backward"]["median_us"], 2)
    res["layer_peak_MB_above_inputs"] = peak_above_inputs(layer_fb, dev)
    res["composition_peak_MB_above_inputs"] = peak_above_inputs(comp_fb, dev)
    with torch.no_grad():
        res["composition_forward_peak_MB_above_inputs"] = peak_above_inputs(lambda: RS.compose(x, flow), dev)
        res["layer_forward_peak_MB_above_inputs"] = peak_above_inputs(lambda: layer(x, flow), dev)
    a.grad = f.grad = None
    return res


def flow_sweep(shape, dev, gen, n_windows, calls):
    B, C, H, W = shape
    x = torch.randn(shape, generator=gen).to(dev)
    out = torch.empty_like(x)
    flows = {"zero": RS.flow_family("zero", B, H, W), "half_pixel": np.full((B, 2, H, W), 0.5, np.float32),
             "smooth_integer_rows": RS.flow_family("smooth", B, H, W), "smooth": RS.flow_family("smooth", B, H, W)}
    flows["smooth_integer_rows"][:, 1] = np.rint(flows["smooth_integer_rows"][:, 1])
    res = {}
    for name, fl in flows.items():
        f = torch.from_numpy(fl).to(dev)
        r = windows({"general": lambda: fn2_capi.forward_warp_forward(x, f, fn2_capi.FN2S_GENERAL, out=out),
                     "tiled": lambda: fn2_capi.forward_warp_forward(x, f, fn2_capi.FN2S_TILED, out=out),
                     "clear_only": lambda: out.zero_()}, n_windows, calls)
        res[name] = {k: v["median_us"] for k, v in r.items()}
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
    res = {"device": torch.cuda.get_device_name(0), "windows": a.windows, "calls_per_window": a.calls, "unit": "microseconds per call",
           "copy_ceiling_GBps": round(ceiling, 1), "atomic_rate_GBps_assumed": ATOMIC_GBPS, "rows": {}}
    for shape in ROWS:
        for family in FAMILIES:
            name = "x".join(map(str, shape)) + "_" + family
            r = row(shape, family, dev, gen, ceiling, a.windows, a.calls)
            res["rows"][name] = r
            print(f"{name:24s} fwd general {r['forward_general']['median_us']:8.1f} tiled {r['forward_tiled']['median_us']:8.1f} det "
                  f"{r['forward_deterministic']['median_us']:8.1f} composition {r['composition_forward']['median_us']:8.1f} us | bwd "
                  f"{r['backward']['median_us']:8.1f} us | fwd + bwd layer {r['layer_forward_backward']['median_us']:8.1f} composition "
                  f"{r['composition_forward_backward']['median_us']:8.1f} us | atomic B / input B {r['forward_general']['atomic_bytes_per_input_byte']} / "
                  f"{r['forward_tiled']['atomic_bytes_per_input_byte']} | peak {r['layer_peak_MB_above_inputs']} / "
                  f"{r['composition_peak_MB_above_inputs']} MB", file=sys.stderr, flush=True)
            if a.quick:
                break
        if a.quick:
            break
    if not a.quick:
        res["flow_sweep_median_us"] = {"x".join(map(str, shape)): flow_sweep(shape, dev, gen, a.windows, a.calls) for shape in ROWS}
        print(json.dumps(res["flow_sweep_median_us"]), file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
