"""The ternary census distance (float32): the layer against what a user writes without it -- the identity-filter ``conv2d`` unfold,
the soft sign, the robust distance, the mean and the border mask -- and against the chip's copy rate, in ONE process: machines
differ by up to 20 %, so a number from another run is not a baseline.

Rows: 8 x 3 x 384 x 512 with max_distance 3 (ARFlow, 49 taps) and 1 (9 taps), im2 = im1 + 5 % noise as in the tests.  Per row:
the forward and the backward (both gradients, and im2's alone, the one a warped second frame needs) through the C ABI on
preallocated tensors, the composition's forward and forward + backward through autograd and the layer's forward + backward, HIP
events around windows of K calls, the contestants alternating window by window, median / min / max window as microseconds per
call; the peak memory above the inputs of both; the bytes the operation has to move (two images in, one plane out; the backward
the two images and grad_out in, two gradients out) with the time they take at the copy rate measured in this process; and the
time the tap loop's instructions take to issue -- per tap and wave, 3 transcendental instructions of 8 cycles among the plain VALU
instructions of 4 cycles counted in the kernels' ISA -- on the device's SIMDs at its clock.  The kernel is bound by whichever of
the two floors is the higher one; the JSON says which.

    python scripts/bench_census.py [--out profiles/census_micro.json] [--windows 7] [--calls 10] [--quick]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import census_ref as RC  # noqa: E402
import fn2_capi  # noqa: E402
from bench_corr_dense import copy_ceiling, windows  # noqa: E402

ROWS = [((8, 3, 384, 512), 3), ((8, 3, 384, 512), 1)]
SCALE = 255.0
# vector instructions per tap and wave in the rolled dx loop of the md = 3 kernels (hipcc -save-temps, gfx950): per 28 taps the
# forward issues 84 transcendental instructions and 354 others (318 VALU, 130 of them packed, and 36 s_nop), the backward with
# both gradients 84 and 588 (548 VALU, 300 of them packed, and 40 s_nop); a packed instruction is counted as 4 cycles like a plain one
ISSUE_CYCLES_PER_TAP = {"forward": (84 * 8 + 354 * 4) / 28.0, "backward": (84 * 8 + 588 * 4) / 28.0}
TRANS_CYCLES_PER_TAP = 3 * 8.0


def peak_above_inputs(fn, dev):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)


def issue_floor_us(shape, md, cycles_per_tap, dev):
    """Microseconds the tap loop needs if every SIMD issues one vector instruction stream without a stall: waves x taps x cycles."""
    N, C, H, W = shape
    m = RC.header_macros()
    tiles = N * -(-H // m["FN2C_TILE_H"]) * -(-W // m["FN2C_TILE_W"])
    waves = tiles * m["FN2C_TILE_H"] * m["FN2C_TILE_W"] // 64
    props = torch.cuda.get_device_properties(dev)
    simds = 4 * props.multi_processor_count
    khz = getattr(props, "clock_rate", 2400000)
    return waves * (2 * md + 1) ** 2 * cycles_per_tap / simds / (khz * 1e3) * 1e6


def row(shape, md, dev, ceiling, n_windows, calls):
    from networks.census_package import TernaryCensus
    N, C, H, W = shape
    im1, im2, go = (torch.from_numpy(a).to(dev) for a in RC.image_pair(shape, 17))
    out = torch.empty(N, 1, H, W, device=dev)
    g1, g2 = torch.empty_like(im1), torch.empty_like(im2)
    # the two must be the same function before their times mean anything
    with torch.no_grad():
        ref = RC.compose(im1, im2, md, SCALE)
        got = fn2_capi.census_forward(im1, im2, md, SCALE, True)
        assert float((got - ref).abs().max()) <= 1e-4, "layer and composition differ"
    a, b = im1.clone().requires_grad_(True), im2.clone().requires_grad_(True)
    layer = TernaryCensus(md, SCALE)
    RC.compose(a, b, md, SCALE).backward(go)
    ca, cb = a.grad.clone(), b.grad.clone()
    a.grad = b.grad = None
    layer(a, b).backward(go)
    for got, want in ((a.grad, ca), (b.grad, cb)):
        assert float((got - want).abs().max()) <= 1e-3 * float(want.abs().max()), "layer and composition gradients differ"

    def comp_fb():
        a.grad = b.grad = None
        RC.compose(a, b, md, SCALE).backward(go)

    def layer_fb():
        a.grad = b.grad = None
        layer(a, b).backward(go)

    with torch.no_grad():
        res = windows({"forward": lambda: fn2_capi.census_forward(im1, im2, md, SCALE, True, out=out),
                       "backward": lambda: fn2_capi.census_backward(im1, im2, go, md, SCALE, True, grads=(g1, g2)),
                       "backward_im2_only": lambda: fn2_capi.census_backward(im1, im2, go, md, SCALE, True, want1=False, grads=(None, g2)),
                       "composition_forward": lambda: RC.compose(im1, im2, md, SCALE)}, n_windows, calls)
    res.update(windows({"layer_forward_backward": layer_fb, "composition_forward_backward": comp_fb}, n_windows, calls))
    in_bytes = 4 * N * C * H * W
    plane = 4 * N * H * W
    moved = {"forward": 2 * in_bytes + plane, "backward": 4 * in_bytes + plane}
    for part, nbytes in moved.items():
        t = res[part]["median_us"]
        bw_floor = nbytes / (ceiling * 1e9) * 1e6
        issue = issue_floor_us(shape, md, ISSUE_CYCLES_PER_TAP[part], dev)
        trans = issue_floor_us(shape, md, TRANS_CYCLES_PER_TAP, dev)
        res[part].update({"algorithmic_MB": round(nbytes / 1e6, 1), "copy_floor_us": round(bw_floor, 1),
                          "share_of_copy_ceiling": round(bw_floor / t, 3), "transcendental_floor_us": round(trans, 1),
                          "vector_issue_floor_us": round(issue, 1), "share_of_vector_issue_rate": round(issue / t, 3),
                          "bound_by": "vector issue (transcendental and plain VALU instructions)" if issue > bw_floor else "memory bandwidth"})
    res["input_MB"] = round(2 * in_bytes / 1e6, 1)
    res["composition_over_layer_forward"] = round(res["composition_forward"]["median_us"] / res["forward"]["median_us"], 2)
    res["composition_over_layer_forward_backward"] = round(res["composition_forward_backward"]["median_us"] /
                                                           res["layer_forward_backward"]["median_us"], 2)
    res["layer_peak_MB_above_inputs"] = peak_above_inputs(layer_fb, dev)
    res["composition_peak_MB_above_inputs"] = peak_above_inputs(comp_fb, dev)
    with torch.no_grad():
        res["composition_forward_peak_MB_above_inputs"] = peak_above_inputs(lambda: RC.compose(im1, im2, md, SCALE), dev)
        res["layer_forward_peak_MB_above_inputs"] = peak_above_inputs(lambda: layer(im1, im2), dev)
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
    props = torch.cuda.get_device_properties(dev)
    res = {"device": torch.cuda.get_device_name(0), "windows": a.windows, "calls_per_window": a.calls, "unit": "microseconds per call",
           "copy_ceiling_GBps": round(ceiling, 1), "compute_units": props.multi_processor_count,
           "clock_MHz": round(getattr(props, "clock_rate", 2400000) / 1e3), "rows": {}}
    for shape, md in ROWS[:1 if a.quick else None]:
        name = "x".join(map(str, shape)) + f"_md{md}"
        r = row(shape, md, dev, ceiling, a.windows, a.calls)
        res["rows"][name] = r
        print(f"{name:22s} fwd {r['forward']['median_us']:8.1f} composition {r['composition_forward']['median_us']:9.1f} us | bwd "
              f"{r['backward']['median_us']:8.1f} (im2 only {r['backward_im2_only']['median_us']:8.1f}) us | fwd + bwd layer "
              f"{r['layer_forward_backward']['median_us']:8.1f} composition {r['composition_forward_backward']['median_us']:9.1f} us | floors fwd "
              f"copy {r['forward']['copy_floor_us']} issue {r['forward']['vector_issue_floor_us']} us | peak "
              f"{r['layer_peak_MB_above_inputs']} / {r['composition_peak_MB_above_inputs']} MB", file=sys.stderr, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
