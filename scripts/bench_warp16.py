"""The fused warp rows on 16-bit tensors: the native kernels (fn2_warp_diff_norm*_16 through the modules) against the widened
composition they replace, `row(x.float(), flow.float()).to(dtype)`, in ONE process -- machines differ by up to 20 %, so a number from
another run is not a baseline.  Half and bfloat16, both rows (WarpDiffNormCat, WarpDiffNorm), 8 x 6 x 384 x 512, forward (no grad) and
forward + flow-gradient backward.  Device events around windows of K calls, the two variants alternating window by window; each entry
reports the median, min and max window as microseconds per call.

    python scripts/bench_warp16.py [--out profiles/warp16_micro.json] [--windows 9] [--calls 20]

Exit status 1 if a forward case misses the bar: the slowest native window must be faster than the fastest composition window.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd")]

import torch  # noqa: E402

SHAPE = (8, 6, 384, 512)


def windows(fns, n_windows, calls, warm=3):
    """fns: {name: callable}; windows of `calls` back-to-back calls, the variants alternating; us per call: median, min, max"""
    for _ in range(warm):
        for f in fns.values():
            for _ in range(calls):
                f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(n_windows):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(calls):
                f()
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e) * 1e3 / calls)
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    return out


def cases(dt, dev):
    from networks.resample2d_package.resample2d import WarpDiffNorm, WarpDiffNormCat
    B, C2, H, W = SHAPE
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(SHAPE, generator=g) - 0.5).to(dt).to(dev)
    flow = (torch.randn(B, 2, H, W, generator=g) * 4.0).to(dt).to(dev)
    fg = flow.clone().requires_grad_(True)
    res = {}
    for name, mod, oc in (("cat", WarpDiffNormCat(20.0), C2 + C2 // 2 + 3), ("norm", WarpDiffNorm(), 1)):
        go = torch.randn(B, oc, H, W, generator=g).to(dt).to(dev)

        def fwd_native(mod=mod):
            with torch.no_grad():
                return mod(x, flow)

        def fwd_widened(mod=mod):
            with torch.no_grad():
                return mod(x.float(), flow.float()).to(dt)

        def fb_native(mod=mod, go=go):
            fg.grad = None
            mod(x, fg).backward(go)

        def fb_widened(mod=mod, go=go):
            fg.grad = None
            mod(x.float(), fg.float()).to(dt).backward(go)

        assert torch.equal(fwd_native().view(torch.int16), fwd_widened().view(torch.int16)), "native and widened rows differ"
        res[name + "_forward"] = {"native": fwd_native, "widened": fwd_widened}
        res[name + "_forward_backward"] = {"native": fb_native, "widened": fb_widened}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert a.windows >= 7, "at least 7 windows per variant"
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "windows": a.windows, "calls_per_window": a.calls,
           "unit": "microseconds per call"}
    ok = True
    for dname, dt in (("half", torch.float16), ("bf16", torch.bfloat16)):
        for cname, fns in cases(dt, dev).items():
            r = windows(fns, a.windows, a.calls)
            r["widened_over_native_median"] = round(r["widened"]["median_us"] / r["native"]["median_us"], 2)
            if cname.endswith("_forward"):
                r["bar_native_max_below_widened_min"] = r["native"]["max_us"] < r["widened"]["min_us"]
                ok = ok and r["bar_native_max_below_widened_min"]
            res[dname + "_" + cname] = r
    res["forward_bar_met"] = ok
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
