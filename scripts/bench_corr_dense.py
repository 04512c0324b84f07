"""Dense stride-1 cost volumes, Correlation(4, 1, 4, 1, 1): FN2_CORR_AUTO (the LDS-tiled kernels of csrc/correlation_dense.hip)
against FN2_CORR_DIRECT (the one-lane-per-output kernel every dense call ran before them) in ONE process -- machines differ by up
to 20 %, so a number from another run is not a baseline.  The five PWC-Net pyramid levels of a 384 x 512 input at B = 8 and the
finest one at 112 x 256; float, half, bfloat16; forward, fused forward (LeakyReLU + store into a concat slice), backward.
Device events around windows of K calls, the two kernels alternating window by window; median, min and max window as
microseconds per call.  Per case: the compulsory bytes (every input and output element once), the GB/s AUTO achieves on them
and that as a fraction of the streaming-copy ceiling measured in the same run (fn2_debug_stream_copy, read + write bytes).

    python scripts/bench_corr_dense.py [--out profiles/corr_dense_micro.json] [--windows 7] [--calls 20] [--quick]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd")]

import torch  # noqa: E402

import fn2_capi  # noqa: E402

PARAMS = (4, 1, 4, 1, 1)
NOUT = 81
B = 8
LEVELS = [(196, 6, 8), (128, 12, 16), (96, 24, 32), (64, 48, 64), (32, 96, 128), (32, 112, 256)]   # C, H, W
DTYPES = (("f32", torch.float32), ("half", torch.float16), ("bf16", torch.bfloat16))


def windows(fns, n_windows, calls, warm=2):
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


def copy_ceiling(dev):
    """GB/s (read + write) of the float4 grid-stride copy of 1 GiB: best of a few grid sizes, temporal and non-temporal."""
    dl = fn2_capi.debug_lib()
    src = torch.empty(1 << 28, device=dev, dtype=torch.float32)
    dst = torch.empty_like(src)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    best = 0.0
    for blocks in (2048, 4096, 8192, 16384):
        for nt in (0, 1):
            def run():
                fn2_capi.check(dl.fn2_debug_stream_copy(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                                        ctypes.c_size_t(src.numel() * 4), blocks, nt, st), "fn2_debug_stream_copy")
            run()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(3)]
            for s, e in ev:
                s.record(); run(); e.record()
            torch.cuda.synchronize()
            best = max(best, 2 * src.numel() * 4 / (min(s.elapsed_time(e) for s, e in ev) * 1e-3) / 1e9)
    return best


def cases(C, H, W, dt, dev):
    g = torch.Generator().manual_seed(C + H + W)
    a = torch.randn(B, C, H, W, generator=g).to(dt).to(dev)
    b = torch.randn(B, C, H, W, generator=g).to(dt).to(dev)
    out = torch.empty(B, NOUT, H, W, dtype=dt, device=dev)
    buf = torch.zeros(B, C + NOUT, H, W, dtype=dt, device=dev)     # the decoder's concat buffer: features, then the cost volume
    go = torch.randn(B, NOUT, H, W, generator=g).to(dt).to(dev)
    g12 = (torch.empty_like(a), torch.empty_like(b))
    es = a.element_size()
    n_in, n_out = a.numel() * es, out.numel() * es
    A, D = fn2_capi.FN2_CORR_AUTO, fn2_capi.FN2_CORR_DIRECT
    # AUTO and DIRECT must agree bit for bit before their times mean anything
    ref = fn2_capi.correlation_forward(a, b, *PARAMS, algo=D)
    assert torch.equal(fn2_capi.correlation_forward(a, b, *PARAMS, algo=A), ref), "AUTO and FN2_CORR_DIRECT differ"
    return {
        "forward": (2 * n_in + n_out, {k: (lambda al=al: fn2_capi.correlation_forward(a, b, *PARAMS, algo=al, out=out))
                                       for k, al in (("auto", A), ("direct", D))}),
        "forward_fused": (2 * n_in + n_out, {k: (lambda al=al: fn2_capi.correlation_forward_fused(a, b, buf, C, 0.1, *PARAMS, algo=al))
                                             for k, al in (("auto", A), ("direct", D))}),
        "backward": (4 * n_in + n_out, {k: (lambda al=al: fn2_capi.correlation_backward(a, b, go, *PARAMS, algo=al, out=g12))
                                        for k, al in (("auto", A), ("direct", D))}),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="float32 and half only, the two finest levels")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    ceiling = copy_ceiling(dev)
    res = {"device": torch.cuda.get_device_name(0), "params": list(PARAMS), "batch": B, "windows": a.windows,
           "calls_per_window": a.calls, "unit": "microseconds per call", "copy_ceiling_GBps": round(ceiling, 1), "cases": {}}
    levels = LEVELS[-3:-1] if a.quick else LEVELS
    dtypes = DTYPES[:2] if a.quick else DTYPES
    for dname, dt in dtypes:
        for (C, H, W) in levels:
            for cname, (nbytes, fns) in cases(C, H, W, dt, dev).items():
                r = windows(fns, a.windows, a.calls)
                gbs = nbytes / (r["auto"]["median_us"] * 1e-6) / 1e9
                r.update(compulsory_MB=round(nbytes / 1e6, 2), auto_GBps=round(gbs, 1), fraction_of_copy_ceiling=round(gbs / ceiling, 3),
                         byte_floor_us=round(nbytes / (ceiling * 1e9) * 1e6, 2),
                         direct_over_auto_median=round(r["direct"]["median_us"] / r["auto"]["median_us"], 2),
                         auto_max_below_direct_min=r["auto"]["max_us"] < r["direct"]["min_us"])
                res["cases"][f"{dname}_{C}x{H}x{W}_{cname}"] = r
                print(f"{dname:5s} {C:3d}x{H:3d}x{W:3d} {cname:14s} auto {r['auto']['median_us']:8.1f} us  direct "
                      f"{r['direct']['median_us']:8.1f} us  x{r['direct_over_auto_median']:.2f}  floor {r['byte_floor_us']:.1f} us",
                      file=sys.stderr)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
