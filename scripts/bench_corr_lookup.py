"""CorrLookup (r = 4, B = 8, C = 256, float32): the general kernels (FN2L_LOOKUP_GENERAL) against the staged ones
(FN2L_LOOKUP_STAGED) in ONE process -- machines differ by up to 20 %, so a number from another run is not a baseline -- and
against what a user writes without the layer: RAFT's all-pairs volume, pooled into a pyramid, and grid_sample.

Maps 48 x 64 and 55 x 128 (Sintel at 1/8), four pyramid levels each (fmap2 pooled with avg_pool2d, coords / 2^level); the
coordinates are the identity plus a smooth flow of up to 3 pixels, and one more row at 48 x 64, level 0, has uniform random
coordinates (every tile of the staged kernels falls back to the general code).  Per row: forward general / staged; backward
(grad_fmap1 + the clear + grad_fmap2's atomic scatter) general / staged, HIP events around windows of K calls, the contestants
alternating window by window, median / min / max window as microseconds per call; the backward's split into its kernels from
the profiler's device times (mean per call, one window); grad_fmap2's atomic bytes (4 B per add, grid points inside fmap2 only)
over its time against the chip-wide float-atomic rate of 1.3 TB/s.  Per map: the composition's build (matmul + pooling, once per
image pair), its lookup (four grid_sample calls, once per iteration), build + lookup + backward, its max_memory_allocated, and
the layer's for four levels forward + backward.

    python scripts/bench_corr_lookup.py [--out profiles/corr_lookup_micro.json] [--windows 7] [--calls 10] [--quick]
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

import fn2_capi  # noqa: E402
from bench_corr_dense import windows  # noqa: E402
from corr_lookup_ref import compose  # noqa: E402

B, C, R, LEVELS = 8, 256, 4, 4
MAPS = [(48, 64), (55, 128)]
ATOMIC_RATE = 1.3e12   # bytes of float atomic adds per second, chip-wide (the guide's measured rate)
G, S = fn2_capi.FN2L_LOOKUP_GENERAL, fn2_capi.FN2L_LOOKUP_STAGED
SCALE = C ** -0.5


def smooth_coords(H, W, dev, gen):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ph = torch.rand(B, 2, 1, 1, generator=gen) * 6.28
    flow = 2.9 * torch.sin(0.11 * xs + 0.07 * ys + ph) * torch.cos(0.05 * ys - ph)
    return (torch.stack([xs, ys])[None] + flow).contiguous().to(dev)


def atomic_bytes(co, H2, W2):
    """4 B per (pixel, channel, grid point inside fmap2)."""
    x0, y0 = torch.floor(co[:, 0]).long(), torch.floor(co[:, 1]).long()
    nx = (torch.clamp(x0 + R + 2, max=W2) - torch.clamp(x0 - R, min=0)).clamp(min=0)
    ny = (torch.clamp(y0 + R + 2, max=H2) - torch.clamp(y0 - R, min=0)).clamp(min=0)
    return int((nx * ny).sum()) * C * 4


def kernel_split(fn, calls):
    """Mean device microseconds per call of the kernels of `fn`, by name, from torch.profiler; {} if it reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            name = "grad_fmap1" if "lookup_g1" in ev.key else "grad_fmap2" if "lookup_g2" in ev.key else "clear" if "emset" in ev.key or "fill" in ev.key.lower() else None
            if name and t:
                out[name] = round(out.get(name, 0.0) + t / calls, 2)
        return out
    except Exception as e:   # the profiler is an aid here, not the measurement
        return {"error": repr(e)[:200]}


def layer_row(f1, f2, co, n_windows, calls):
    D2 = (2 * R + 1) ** 2
    Bn, _, H, W = f1.shape
    out = torch.empty(Bn, D2, H, W, device=f1.device)
    go = torch.randn(Bn, D2, H, W, device=f1.device)
    g12 = (torch.empty_like(f1), torch.empty_like(f2))
    # the two kernels must agree bit for bit before their times mean anything
    ref = fn2_capi.corr_lookup_forward(f1, f2, co, R, SCALE, algo=G)
    assert torch.equal(fn2_capi.corr_lookup_forward(f1, f2, co, R, SCALE, algo=S), ref), "staged and general forward differ"
    r1, _ = fn2_capi.corr_lookup_backward(f1, f2, co, go, R, SCALE, algo=G)
    s1, _ = fn2_capi.corr_lookup_backward(f1, f2, co, go, R, SCALE, algo=S)
    assert torch.equal(s1, r1), "staged and general grad_fmap1 differ"
    row = {"forward": windows({k: (lambda al=al: fn2_capi.corr_lookup_forward(f1, f2, co, R, SCALE, algo=al, out=out))
                               for k, al in (("general", G), ("staged", S))}, n_windows, calls),
           "backward": windows({k: (lambda al=al: fn2_capi.corr_lookup_backward(f1, f2, co, go, R, SCALE, algo=al, out=g12))
                                for k, al in (("general", G), ("staged", S))}, n_windows, calls)}
    for k, al in (("general", G), ("staged", S)):
        row["backward"][k]["kernels_us"] = kernel_split(lambda al=al: fn2_capi.corr_lookup_backward(f1, f2, co, go, R, SCALE, algo=al, out=g12), calls)
    nbytes = atomic_bytes(co, f2.shape[2], f2.shape[3])
    t2 = row["backward"]["general"]["kernels_us"].get("grad_fmap2")
    row["grad_fmap2_atomic_MB"] = round(nbytes / 1e6, 1)
    row["grad_fmap2_atomic_floor_us"] = round(nbytes / ATOMIC_RATE * 1e6, 1)
    if t2:
        row["grad_fmap2_atomic_GBps"] = round(nbytes / (t2 * 1e-6) / 1e9, 1)
        row["grad_fmap2_fraction_of_atomic_rate"] = round(nbytes / (t2 * 1e-6) / ATOMIC_RATE, 3)
    for part in ("forward", "backward"):
        row[part]["general_over_staged_median"] = round(row[part]["general"]["median_us"] / row[part]["staged"]["median_us"], 2)
    return row


def composition_rows(f1, f2, co, dev):
    """The PyTorch composition over the whole pyramid: build, lookup, forward + backward, and its peak memory."""
    def build():
        Bn, Cn, H, W = f1.shape
        corr = torch.matmul(f1.reshape(Bn, Cn, H * W).transpose(1, 2), f2.reshape(Bn, Cn, -1)) * SCALE
        pyr = [corr.reshape(Bn * H * W, 1, *f2.shape[2:])]
        for _ in range(LEVELS - 1):
            pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
        return pyr

    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    go = torch.randn(f1.shape[0], LEVELS * (2 * R + 1) ** 2, f1.shape[2], f1.shape[3], device=dev)

    def fwd_bwd():
        a.grad = b.grad = None
        compose(a, b, co, R, SCALE, num_levels=LEVELS).backward(go)

    with torch.no_grad():
        res = windows({"composition_forward": lambda: compose(f1, f2, co, R, SCALE, num_levels=LEVELS), "composition_build": build}, 3, 2, warm=1)
    res.update(windows({"composition_forward_backward": fwd_bwd}, 3, 1, warm=1))
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fwd_bwd()
    torch.cuda.synchronize()
    res["composition_peak_MB_above_inputs"] = round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)
    a.grad = b.grad = None
    return res


def layer_memory(f1, f2, co, dev):
    from networks.correlation_package import AlternateCorrBlock
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    go = torch.randn(f1.shape[0], LEVELS * (2 * R + 1) ** 2, f1.shape[2], f1.shape[3], device=dev)

    def fwd_bwd():
        a.grad = b.grad = None
        AlternateCorrBlock(a, b, num_levels=LEVELS, radius=R)(co).backward(go)

    res = windows({"layer_forward_backward": fwd_bwd}, 3, 2, warm=1)
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fwd_bwd()
    torch.cuda.synchronize()
    res["layer_peak_MB_above_inputs"] = round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="the 48 x 64 map only, no composition")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "channels": C, "radius": R, "levels": LEVELS, "windows": a.windows,
           "calls_per_window": a.calls, "unit": "microseconds per call", "atomic_rate_GBps": ATOMIC_RATE / 1e9,
           "composition": "3 windows of 2 calls (forward + backward: of 1)", "rows": {}, "maps": {}}
    for (H, W) in (MAPS[:1] if a.quick else MAPS):
        f1 = torch.randn(B, C, H, W, generator=gen).to(dev)
        f2 = torch.randn(B, C, H, W, generator=gen).to(dev)
        co = smooth_coords(H, W, dev, gen)
        pyr = [f2]
        for _ in range(LEVELS - 1):
            pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
        rows = [(f"{H}x{W}_level{i}_smooth", lvl, (co / 2 ** i).contiguous()) for i, lvl in enumerate(pyr)]
        if (H, W) == MAPS[0]:
            rnd = torch.stack([torch.rand(B, H, W, generator=gen) * W, torch.rand(B, H, W, generator=gen) * H], 1).to(dev)
            rows.append((f"{H}x{W}_level0_random", f2, rnd))
        for name, lvl, c in rows:
            r = layer_row(f1, lvl, c, a.windows, a.calls)
            r["fmap2"] = list(lvl.shape[2:])
            r["tiles"] = B * math.ceil(W / 16) * math.ceil(H / 4)
            res["rows"][name] = r
            k = r["backward"]["general"]["kernels_us"]
            print(f"{name:26s} fwd general {r['forward']['general']['median_us']:8.1f} staged {r['forward']['staged']['median_us']:8.1f} us | "
                  f"bwd general {r['backward']['general']['median_us']:8.1f} staged {r['backward']['staged']['median_us']:8.1f} us | "
                  f"g1 {k.get('grad_fmap1')} / staged {r['backward']['staged']['kernels_us'].get('grad_fmap1')}  g2 {k.get('grad_fmap2')} us, "
                  f"atomic floor {r['grad_fmap2_atomic_floor_us']} us", file=sys.stderr, flush=True)
        m = layer_memory(f1, f2, co, dev)
        if not a.quick:
            m.update(composition_rows(f1, f2, co, dev))
        m["all_pairs_volume_MB"] = round(B * (H * W) ** 2 * 4 / 1e6, 1)
        res["maps"][f"{H}x{W}"] = m
        print(f"{H}x{W}: {m}", file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
