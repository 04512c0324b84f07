#!/usr/bin/env python3
"""Which kernels the correlation dispatcher launches: every call of tests/corr_dispatch_cases.py whose plan is a list of kernels, once,
in the table's order, through the entry point the case speaks of (fn2_correlation_forward_ex / _forward_fused for a batch stride,
_backward_ex, and fn2_debug_correlation_* for a variant), on tensors at the case's addresses modulo 16.  No timing, no repetition:

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/corr_dispatch_trace.py --lib DIR
  python scripts/corr_dispatch_trace.py --list OUT/.../*_kernel_trace.csv      # the ordered kernel list (name, grid, workgroup)

with two builds (DIR holds libflownet2_hip.so and libflownet2_hip_debug.so; default: this tree's), and compare the two lists.
"""
import argparse
import csv
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "flownet2-pytorch_amd"), os.path.join(ROOT, "tests")]


def kernel_list(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print("%s grid %s,%s,%s wg %s,%s,%s" % ((r["Kernel_Name"],) + tuple(r["Grid_Size_" + a] for a in "XYZ") +
                                                tuple(r["Workgroup_Size_" + a] for a in "XYZ")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="directory of another build's libflownet2_hip.so and libflownet2_hip_debug.so")
    ap.add_argument("--list", help="print the ordered kernel list of a rocprofv3 kernel-trace CSV and exit")
    a = ap.parse_args()
    if a.list:
        return kernel_list(a.list)
    import torch
    import fn2_capi
    import corr_dispatch_cases as cases
    if a.lib:
        fn2_capi.LIB_PATH = os.path.join(os.path.abspath(a.lib), "libflownet2_hip.so")
        fn2_capi.DEBUG_LIB_PATH = os.path.join(os.path.abspath(a.lib), "libflownet2_hip_debug.so")
    lib, dbg = fn2_capi.lib(), fn2_capi.debug_lib()
    tdtype = {cases.F32: torch.float32, cases.HALF: torch.float16, cases.BF16: torch.bfloat16, cases.F64: torch.float64}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = []

    def dev(n, dtype, address, seed):
        """n random elements on the GPU (made on the host: no kernel of torch's), at `address` modulo 16"""
        es = torch.empty(0, dtype=dtype).element_size()
        buf = torch.empty(n + 16 // es, dtype=dtype, device="cuda")
        off = ((address - buf.data_ptr()) % 16) // es
        buf[off:off + n].copy_(torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(dtype))
        keep.append(buf)
        return ctypes.c_void_p(buf.data_ptr() + off * es)

    for i, (what, direction, dtype, shape, params, kw, want) in enumerate(cases.FORWARD_AUTO + cases.FORWARD_FORCED + cases.BACKWARD_AUTO + cases.DEBUG):
        if isinstance(want, int):
            continue
        B, C, H, W = shape
        n_in, n_out = B * C * H * W, fn2_capi.correlation_output_shape(H, W, *params)
        n_out, out_bs = n_out[0] * n_out[1] * n_out[2], kw.get("out_bs", 0)
        algo, addr = kw.get("algo", fn2_capi.FN2_CORR_AUTO), kw.get("ptrs", (cases.A16,) * 5)
        in1, in2 = dev(n_in, tdtype[dtype], addr[0], 2 * i), dev(n_in, tdtype[dtype], addr[1], 2 * i + 1)
        third = dev(B * max(out_bs, n_out), tdtype[dtype], addr[2], 1000 + i)            # the output / the output's gradient
        tail = (dtype, B, C, H, W) + params + (algo, stream)
        if direction == "backward":
            g1, g2 = dev(n_in, tdtype[dtype], addr[3], 0), dev(n_in, tdtype[dtype], addr[4], 0)
            rc = (dbg.fn2_debug_correlation_backward if algo >= 100 else lib.fn2_correlation_backward_ex)(in1, in2, third, g1, g2, *tail)
        elif out_bs:
            rc = lib.fn2_correlation_forward_fused(in1, in2, third, ctypes.c_int64(out_bs), ctypes.c_float(1.0), *tail)
        else:
            rc = (dbg.fn2_debug_correlation_forward if algo >= 100 else lib.fn2_correlation_forward_ex)(in1, in2, third, *tail)
        torch.cuda.synchronize()
        print("%-24s rc %d" % (what, rc), flush=True)   # (a profiling variant may decline a shape: the code is part of the comparison)
    return 0


if __name__ == "__main__":
    sys.exit(main())
