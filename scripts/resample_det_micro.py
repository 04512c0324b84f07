"""Resample2d backward at 8x3x384x512: the default (fp32 atomics) entry point against the deterministic one (fixed-point grad_input1,
fn2_resample2d_backward_det), with bench.py's flow (randn x 4) and a translation of (25, -18) px.  Each time is a device-event pair
around the whole C-ABI call -- for the deterministic one: workspace clearing, plane-maximum prepass, scatter + gather, fallback check and
conversion; for both: the zero fill of grad_input1 the caller owes.  The two entry points alternate inside every repeat; median and min
over warmed repeats.

    python scripts/resample_det_micro.py [--out profiles/resample_det_micro.json] [--reps 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import fn2_capi  # noqa: E402
import resample_det_ref as R  # noqa: E402


def timed(fns, reps, warm=5):
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1000.0)
    return {k: {"median_us": sorted(v)[len(v) // 2], "min_us": min(v)} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = fn2_capi.lib()
    B, C, H, W = 8, 3, 384, 512
    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, C, H, W, generator=g).to(dev)
    gout = torch.randn(B, C, H, W, generator=g).to(dev)
    gimg, gflow = torch.zeros_like(img), torch.empty(B, 2, H, W, device=dev)
    wsb = lib.fn2_resample2d_backward_det_workspace_bytes(B, C, H, W, H, W, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    P = fn2_capi._p
    null = None
    res = {"shape": [B, C, H, W], "workspace_bytes": int(wsb)}
    for name, flow_np in [("bench_flow", R.bench_flow(B, H, W, 0)), ("translated_25_-18", R.translated_flow(B, H, W, 0))]:
        flow = torch.from_numpy(flow_np).to(dev)
        stream = torch.cuda.current_stream().cuda_stream

        def default():
            gimg.zero_()
            fn2_capi.check(lib.fn2_resample2d_backward(P(img), null, P(flow), P(gout), P(gimg), P(gflow), B, C, H, W, H, W, 1, 1,
                                                       fn2_capi.ctypes.c_void_p(stream)), "default")

        def det():
            gimg.zero_()
            fn2_capi.check(lib.fn2_resample2d_backward_det(P(img), null, P(flow), P(gout), P(gimg), P(gflow), B, C, H, W, H, W, 1, 1,
                                                           P(ws), fn2_capi.ctypes.c_size_t(wsb), fn2_capi.ctypes.c_void_p(stream)), "det")

        def fill():
            gimg.zero_()

        res[name] = timed({"default": default, "deterministic": det, "zero_fill_only": fill}, args.reps)
        # the deterministic result repeats bit for bit
        det()
        a = gimg.clone()
        det()
        res[name]["deterministic_repeats_bitwise"] = bool(torch.equal(a.view(torch.int32), gimg.view(torch.int32)))
    res["device"] = torch.cuda.get_device_name(0)
    s = json.dumps(res, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
