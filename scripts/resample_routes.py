#!/usr/bin/env python3
"""Which kernel each float32 warp entry point launches for which shape: one call per entry point and shape on random inputs, shapes
on both sides of every predicate of the host code (tiled / untiled, tile height, C == 3, alignment, image size, pixel stride,
kernel_size, nearest mode, with and without a pair gradient, the deterministic calls).  No timing, no repetition: run it under
`rocprofv3 --kernel-trace` and compare the ordered kernel list (name, grid, workgroup) of two builds.

  python scripts/resample_routes.py [--lib path/to/libflownet2_hip.so]
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flownet2-pytorch_amd"))
import fn2_capi  # noqa: E402

f32, sz, i64 = ctypes.c_float, ctypes.c_size_t, ctypes.c_int64
NULL = ctypes.c_void_p(0)
_keep = []


def dev(n, scale=1.0, offset=0):
    """n random floats on the GPU (made on the host: no kernel), `offset` floats past a 256-byte aligned allocation"""
    t = (torch.randn(n + offset) * scale).cuda()
    _keep.append(t)
    return ctypes.c_void_p(t.data_ptr() + 4 * offset)


def resample_cases():
    # (label, C, H, W, Hi, Wi, pixel stride, pointer offset in floats, kernel_size, bilinear)
    yield "16x32 C=3", 3, 16, 32, 16, 32, 1, 0, 1, 1
    yield "16x32 C=2", 2, 16, 32, 16, 32, 1, 0, 1, 1
    yield "15x32", 3, 15, 32, 15, 32, 1, 0, 1, 1
    yield "16x28", 3, 16, 28, 16, 28, 1, 0, 1, 1
    yield "16x34", 3, 16, 34, 16, 34, 1, 0, 1, 1
    yield "48x64 C=3", 3, 48, 64, 48, 64, 1, 0, 1, 1
    yield "48x64 C=2", 2, 48, 64, 48, 64, 1, 0, 1, 1
    yield "384x4096 C=2 (one image fills the chip: 48-row tiles)", 2, 384, 4096, 384, 4096, 1, 0, 1, 1
    yield "16x32 image + 1 float", 3, 16, 32, 16, 32, 1, 1, 1, 1
    yield "16x32 Hi = H + 1", 3, 16, 32, 17, 32, 1, 0, 1, 1
    yield "16x32 pixel stride 2", 3, 16, 32, 16, 32, 2, 0, 1, 1
    yield "16x32 kernel_size 2", 3, 16, 32, 16, 32, 1, 0, 2, 1
    yield "16x32 nearest", 3, 16, 32, 16, 32, 1, 0, 1, 0


def pair_cases():
    # (label, C, H, W, pointer offset of the pair in floats, bilinear)
    yield "16x32 C=3", 3, 16, 32, 0, 1
    yield "16x32 C=2", 2, 16, 32, 0, 1
    yield "15x32", 3, 15, 32, 0, 1
    yield "16x28", 3, 16, 28, 0, 1
    yield "16x34", 3, 16, 34, 0, 1
    yield "48x64 C=3", 3, 48, 64, 0, 1
    yield "48x64 C=2", 2, 48, 64, 0, 1
    yield "384x4096 C=2 (48-row tiles)", 2, 384, 4096, 0, 1
    yield "16x32 pair + 1 float", 3, 16, 32, 1, 1
    yield "16x32 nearest", 3, 16, 32, 0, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build of libflownet2_hip.so")
    a = ap.parse_args()
    if a.lib:
        fn2_capi.LIB_PATH = os.path.abspath(a.lib)
    lib = fn2_capi.lib()
    torch.manual_seed(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B = 1
    bad = 0

    def call(what, fn, *args):
        nonlocal bad
        rc = fn(*args)
        torch.cuda.synchronize()
        bad += rc != 0
        print("%-78s rc %d" % (what, rc))

    for label, C, H, W, Hi, Wi, ws, off, ks, bil in resample_cases():
        st = (i64 * 4)(C * Hi * Wi * ws, Hi * Wi * ws, Wi * ws, ws) if ws != 1 else None
        img, flow, gout = dev(B * C * Hi * Wi * ws, offset=off), dev(B * 2 * H * W, 2.0), dev(B * C * H * W)
        out, gimg, gflow = dev(B * C * H * W), dev(B * C * Hi * Wi), dev(B * 2 * H * W)
        dims = (B, C, Hi, Wi, H, W, ks, bil)
        call("resample2d_forward   " + label, lib.fn2_resample2d_forward, img, st, flow, out, *dims, stream)
        call("resample2d_backward  " + label, lib.fn2_resample2d_backward, img, st, flow, gout, gimg, gflow, *dims, stream)
        if label in ("16x32 C=3", "16x32 C=2", "15x32", "16x32 kernel_size 2"):
            need = lib.fn2_resample2d_backward_det_workspace_bytes(B, C, Hi, Wi, H, W, ks)
            wsb = dev(need // 4 + 1)
            call("resample2d_backward_det " + label, lib.fn2_resample2d_backward_det, img, st, flow, gout, gimg, gflow, *dims, wsb, sz(need),
                 stream)
    for label, C, H, W, off, bil in pair_cases():
        HW, CC = H * W, 3 * C + 3
        pair, flow = dev(B * 2 * C * HW, offset=off), dev(B * 2 * HW, 2.0)
        cat, gcat, gpair, gflow = dev(B * CC * HW), dev(B * CC * HW), dev(B * 2 * C * HW), dev(B * 2 * HW)
        nrm, gnrm = dev(B * HW), dev(B * HW)
        dims = (B, C, H, W, bil)
        d20 = f32(20.0)
        call("warp_diff_norm_cat   " + label, lib.fn2_warp_diff_norm_cat, pair, flow, cat, d20, *dims, stream)
        call("warp_diff_norm_cat_backward  grad_pair  " + label, lib.fn2_warp_diff_norm_cat_backward, pair, flow, cat, gcat, gpair, gflow,
             d20, *dims, stream)
        call("warp_diff_norm_cat_backward  no grad_pair  " + label, lib.fn2_warp_diff_norm_cat_backward, pair, flow, cat, gcat, NULL, gflow,
             d20, *dims, stream)
        call("warp_diff_norm       " + label, lib.fn2_warp_diff_norm, pair, flow, nrm, *dims, stream)
        call("warp_diff_norm_backward  " + label, lib.fn2_warp_diff_norm_backward, pair, flow, nrm, gnrm, gflow, *dims, stream)
        if label in ("16x32 C=3", "15x32"):
            need = lib.fn2_warp_diff_norm_cat_backward_det_workspace_bytes(B, C, H, W)
            wsb = dev(need // 4 + 1)
            call("warp_diff_norm_cat_backward_det  grad_pair  " + label, lib.fn2_warp_diff_norm_cat_backward_det, pair, flow, cat, gcat,
                 gpair, gflow, d20, *dims, wsb, sz(need), stream)
            call("warp_diff_norm_cat_backward_det  no grad_pair  " + label, lib.fn2_warp_diff_norm_cat_backward_det, pair, flow, cat, gcat,
                 NULL, gflow, d20, *dims, wsb, sz(need), stream)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
