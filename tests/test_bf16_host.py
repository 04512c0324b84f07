"""CPU-side checks of bfloat16 at the C ABI (FN2_BF16 = 3): the element type is declared and accepted by the correlation and
ChannelNorm entry points -- a call that is wrong in some other way reports that other error, not FN2_EDTYPE -- without an ABI
version change; nothing here launches a kernel."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

import fn2_capi

EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4


def test_bf16_enum_declared_abi_unchanged():
    assert fn2_capi.FN2_BF16 == 3
    hdr = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    assert re.search(r"\bFN2_BF16\s*=\s*3\b", hdr)
    lib = fn2_capi.lib()
    assert lib.fn2_abi_version() == 3
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(fn2_capi.EXPORTS) == sorted(set(re.findall(r"\b(fn2_[a-z0-9_]+)\s*\(", code)))
    assert fn2_capi._dtype_code(torch.empty(0, dtype=torch.bfloat16)) == fn2_capi.FN2_BF16


def test_bf16_calls_report_their_other_errors():
    lib = fn2_capi.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 1)          # odd address: not aligned to a 2-byte element
    i64, f32 = ctypes.c_int64, ctypes.c_float
    # ChannelNorm
    assert lib.fn2_channelnorm_forward(mis, p, 3, 1, 1, 2, 2, null) == EALIGN
    assert lib.fn2_channelnorm_forward(p, p, 3, 1, 0, 2, 2, null) == EINVAL          # C < 1
    assert lib.fn2_channelnorm_forward(p, p, 3, 0, 3, 2, 2, null) == 0               # empty batch: nothing to do
    assert lib.fn2_channelnorm_backward(p, p, mis, null, p, 3, 1, 1, 2, 2, null) == EALIGN
    # correlation forward: every entry point
    assert lib.fn2_correlation_forward(p, p, p, 3, 1, 4, 4, 4, 0, 1, 20, 1, 2, null) == EINVAL      # empty output
    assert lib.fn2_correlation_forward(mis, p, p, 3, 1, 4, 8, 8, 4, 1, 4, 1, 2, null) == EALIGN
    assert lib.fn2_correlation_forward_ex(p, p, mis, 3, 1, 4, 8, 8, 4, 1, 4, 1, 2, 0, null) == EALIGN
    assert lib.fn2_correlation_forward_ex(p, p, p, 3, 1, 4, 8, 8, 4, 1, 4, 1, 2, 99, null) == EINVAL   # unknown selector
    assert lib.fn2_correlation_forward_fused(p, p, p, i64(10), f32(0.1), 3, 1, 4, 8, 8, 4, 1, 4, 1, 2, 0, null) == EINVAL
    assert lib.fn2_correlation_forward_fused(p, p, p, i64(3200), f32(0.1), 3, 0, 4, 8, 8, 4, 1, 4, 1, 2, 0, null) == 0
    # correlation backward: every entry point
    assert lib.fn2_correlation_backward(p, p, p, p, p, 3, 1, 4, 8, 8, 4, 1, 4, 2, 2, null) == EUNSUPPORTED   # stride1 != 1
    assert lib.fn2_correlation_backward(p, p, p, p, mis, 3, 1, 4, 8, 8, 4, 1, 4, 1, 2, null) == EALIGN
    assert lib.fn2_correlation_backward_ex(p, p, p, p, p, 3, 1, 4, 8, 8, 4, 1, 4, 1, 2, -1, null) == EINVAL
    fb = lib.fn2_correlation_backward_fused
    ws = ctypes.c_size_t(1 << 20)
    assert fb(p, p, p, i64(1600), p, i64(1600), f32(0.0), p, ws, p, p, 3, 1, 4, 8, 8, 4, 1, 4, 1, 2, 0, null) == EINVAL  # slope 0
    assert fb(p, p, mis, i64(1600), p, i64(1600), f32(0.1), p, ws, p, p, 3, 1, 4, 8, 8, 4, 1, 4, 1, 2, 0, null) == EALIGN
    # element types past bfloat16 stay unsupported
    for dt in (4, 7):
        assert lib.fn2_channelnorm_forward(p, p, dt, 1, 1, 2, 2, null) == EDTYPE
        assert lib.fn2_channelnorm_backward(p, p, p, null, p, dt, 1, 1, 2, 2, null) == EDTYPE
        assert lib.fn2_correlation_forward(p, p, p, dt, 1, 4, 8, 8, 4, 1, 4, 1, 2, null) == EDTYPE
        assert lib.fn2_correlation_backward(p, p, p, p, p, dt, 1, 4, 8, 8, 4, 1, 4, 1, 2, null) == EDTYPE
        assert fb(p, p, p, i64(1600), p, i64(1600), f32(0.1), p, ws, p, p, dt, 1, 4, 8, 8, 4, 1, 4, 1, 2, 0, null) == EDTYPE


def test_bf16_fused_workspace_is_halfs():
    f = fn2_capi.lib().fn2_correlation_backward_fused_workspace_bytes
    for args in [(2, 48, 64, 20, 1, 20, 1, 2), (1, 8, 8, 4, 1, 4, 1, 2), (3, 10, 12, 3, 3, 2, 1, 1)]:
        n = f(3, *args)
        assert n > 0 and n == f(1, *args) and 2 * n == f(0, *args)
    assert f(4, 2, 48, 64, 20, 1, 20, 1, 2) == 0


@pytest.mark.parametrize("which", ["correlation", "channelnorm", "resample2d"])
def test_bf16_cpu_tensors_meet_the_no_cpu_error(which):
    import channelnorm_cuda
    import correlation_cuda
    import resample2d_cuda
    a = torch.zeros(1, 128, 8, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        if which == "correlation":
            correlation_cuda.apply(a, a.clone(), 20, 1, 20, 1, 2, 1)
        elif which == "channelnorm":
            channelnorm_cuda.apply(a, 2)
        else:
            resample2d_cuda.forward_alloc(a, torch.zeros(1, 2, 8, 8, dtype=torch.bfloat16), 1, True)
