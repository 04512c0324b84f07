"""Correlation1d(pad = md = 40, stride 1): the general kernel (FN2X_CORR1D_GENERAL) against the tiled ones (FN2X_CORR1D_TILED) in
ONE process -- machines differ by up to 20 %, so a number from another run is not a baseline -- and, for float32, against what
the tree offered before the layer: the 2-D Correlation at md 40 sliced to its centre row (6561 channels computed to keep 81)
and the PyTorch composition (pad in2, 81 shifted products, mean over C, stack; backward through autograd).

Shapes at B = 8: a DispNetC-like 128 x 96 x 192 (two-sided and one-sided search), the same map at C = 64 and 32, and two smaller
maps, 48 x 96 and 24 x 48, that place the forward's AUTO gate.  float, half, bfloat16; forward and backward.  Device events
around windows of K calls, the contestants alternating window by window; median, min and max window as microseconds per call.
Per case the algorithmic bytes (the two inputs and the output once; backward: inputs, gradOutput and both gradients once), the
GB/s the faster 1-D kernel achieves on them and that as a fraction of the streaming-copy ceiling measured in the same run
(fn2_debug_stream_copy, read + write bytes: the probe behind bench.py --full's copy_ceiling_GBps).

    python scripts/bench_corr1d.py [--out profiles/corr1d_micro.json] [--windows 7] [--calls 10] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import fn2_capi  # noqa: E402
from bench_corr_dense import copy_ceiling, windows  # noqa: E402

MD = 40
B = 8
CONFIGS = [(128, 96, 192, 0), (128, 96, 192, -1), (64, 96, 192, 0), (32, 96, 192, 0), (128, 48, 96, 0), (128, 24, 48, 0)]   # C, H, W, sd
DTYPES = (("f32", torch.float32), ("half", torch.float16), ("bf16", torch.bfloat16))
G, T = fn2_capi.FN2X_CORR1D_GENERAL, fn2_capi.FN2X_CORR1D_TILED


def composition(a, b):
    W = a.shape[-1]
    bp = torch.nn.functional.pad(b, (MD, MD))
    return torch.stack([(a * bp[..., j:j + W]).mean(1) for j in range(2 * MD + 1)], 1)


def cases(C, H, W, sd, dt, dev, old_ways):
    g = torch.Generator().manual_seed(C + H + W)
    a = torch.randn(B, C, H, W, generator=g).to(dt).to(dev)
    b = torch.randn(B, C, H, W, generator=g).to(dt).to(dev)
    prm = (MD, MD, 1, 1, sd)
    nOut = fn2_capi.correlation1d_output_shape(H, W, *prm)[0]
    out = torch.empty(B, nOut, H, W, dtype=dt, device=dev)
    go = torch.randn(B, nOut, H, W, generator=g).to(dt).to(dev)
    g12 = (torch.empty_like(a), torch.empty_like(b))
    es = a.element_size()
    n_in, n_out = a.numel() * es, out.numel() * es
    # the two kernels must agree bit for bit before their times mean anything
    ref = fn2_capi.correlation1d_forward(a, b, *prm, algo=G)
    assert torch.equal(fn2_capi.correlation1d_forward(a, b, *prm, algo=T), ref), "tiled and general forward differ"
    r1, r2 = fn2_capi.correlation1d_backward(a, b, go, *prm, algo=G)
    t1, t2 = fn2_capi.correlation1d_backward(a, b, go, *prm, algo=T)
    assert torch.equal(t1, r1) and torch.equal(t2, r2), "tiled and general backward differ"
    fwd = {k: (lambda al=al: fn2_capi.correlation1d_forward(a, b, *prm, algo=al, out=out)) for k, al in (("general", G), ("tiled", T))}
    bwd = {k: (lambda al=al: fn2_capi.correlation1d_backward(a, b, go, *prm, algo=al, out=g12)) for k, al in (("general", G), ("tiled", T))}
    res = {"forward": (2 * n_in + n_out, fwd, None), "backward": (4 * n_in + n_out, bwd, None)}
    if old_ways:
        D = 2 * MD + 1
        rows = slice(MD * D, (MD + 1) * D)
        p2 = (MD, 1, MD, 1, 1)
        go2 = torch.zeros(B, D * D, H, W, dtype=dt, device=dev)
        go2[:, rows] = go
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)

        def comp_bwd():
            ar.grad = br.grad = None
            composition(ar, br).backward(go)

        res["forward"] = (2 * n_in + n_out, fwd, {"corr2d_sliced": lambda: fn2_capi.correlation_forward(a, b, *p2)[:, rows].contiguous(),
                                                  "composition": lambda: composition(a, b)})
        res["backward"] = (4 * n_in + n_out, bwd, {"corr2d_sliced": lambda: fn2_capi.correlation_backward(a, b, go2, *p2, out=g12),
                                                   "composition_fwd_bwd": comp_bwd})
    return nOut, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="float32 only, the 32-channel and the smallest map, no 2-D layer / composition")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    ceiling = copy_ceiling(dev)
    res = {"device": torch.cuda.get_device_name(0), "max_displacement": MD, "batch": B, "windows": a.windows, "calls_per_window": a.calls,
           "unit": "microseconds per call", "copy_ceiling_GBps": round(ceiling, 1),
           "old_ways": "float32, two-sided search only; 3 windows of 1 call", "cases": {}}
    configs = [CONFIGS[3], CONFIGS[5]] if a.quick else CONFIGS
    for dname, dt in (DTYPES[:1] if a.quick else DTYPES):
        for (C, H, W, sd) in configs:
            old_ways = dname == "f32" and sd == 0 and not a.quick
            nOut, cs = cases(C, H, W, sd, dt, dev, old_ways)
            tiles = B * ((W + 31) // 32) * ((H + 3) // 4)
            for cname, (nbytes, fns, slow) in cs.items():
                r = windows(fns, a.windows, a.calls)
                if slow:
                    r.update(windows(slow, 3, 1, warm=1))
                best = min(r["general"]["median_us"], r["tiled"]["median_us"])
                gbs = nbytes / (best * 1e-6) / 1e9
                r.update(nOut=nOut, forward_tiles=tiles, algorithmic_MB=round(nbytes / 1e6, 2), best_GBps=round(gbs, 1),
                         fraction_of_copy_ceiling=round(gbs / ceiling, 3), byte_floor_us=round(nbytes / (ceiling * 1e9) * 1e6, 2),
                         general_over_tiled_median=round(r["general"]["median_us"] / r["tiled"]["median_us"], 2),
                         tiled_max_below_general_min=r["tiled"]["max_us"] < r["general"]["min_us"])
                res["cases"][f"{dname}_{C}x{H}x{W}_sd{sd}_{cname}"] = r
                extra = "".join(f"  {k} {r[k]['median_us']:.0f} us" for k in (slow or {}))
                print(f"{dname:5s} {C:3d}x{H:3d}x{W:3d} sd {sd:2d} {cname:9s} general {r['general']['median_us']:9.1f} us  tiled "
                      f"{r['tiled']['median_us']:9.1f} us  x{r['general_over_tiled_median']:.2f}  floor {r['byte_floor_us']:.1f} us{extra}",
                      file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
