"""CPU checks of the 16-bit entry points of the fused warp rows (fn2_warp_diff_norm_cat_16, fn2_warp_diff_norm_cat_backward_16,
fn2_warp_diff_norm_16, fn2_warp_diff_norm_backward_16): the C ABI declares, exports and lists them without a version change, and
rejected calls return their codes before anything touches a device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import fn2_capi

NEW = ["fn2_warp_diff_norm_cat_16", "fn2_warp_diff_norm_cat_backward_16", "fn2_warp_diff_norm_16", "fn2_warp_diff_norm_backward_16"]
OK, EINVAL, EDTYPE, EALIGN = 0, -1, -2, -3
F16, BF16 = fn2_capi.FN2_F16, fn2_capi.FN2_BF16

_buf = (ctypes.c_uint16 * 256)()
P = ctypes.cast(_buf, ctypes.c_void_p)
ODD = ctypes.c_void_p(ctypes.addressof(_buf) + 1)
NULL = ctypes.c_void_p(0)
f32 = ctypes.c_float


def _calls(lib):
    """name -> call(pointers, dtype, div_flow, B, C, H, W): each entry point with its own number of tensor arguments"""
    def cat(p, dt, d, B, C, H, W):
        return lib.fn2_warp_diff_norm_cat_16(p[0], p[1], p[2], dt, f32(d), B, C, H, W, 1, NULL)

    def cat_bwd(p, dt, d, B, C, H, W):
        return lib.fn2_warp_diff_norm_cat_backward_16(p[0], p[1], p[2], p[3], dt, f32(d), B, C, H, W, 1, NULL)

    def norm(p, dt, d, B, C, H, W):
        return lib.fn2_warp_diff_norm_16(p[0], p[1], p[2], dt, B, C, H, W, 1, NULL)

    def norm_bwd(p, dt, d, B, C, H, W):
        return lib.fn2_warp_diff_norm_backward_16(p[0], p[1], p[2], p[3], dt, B, C, H, W, 1, NULL)

    return {"cat": (cat, 3), "cat_bwd": (cat_bwd, 4), "norm": (norm, 3), "norm_bwd": (norm_bwd, 4)}


def test_new_symbols_declared_exported_listed():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flownet2_hip.h")).read(), flags=re.S)
    lib = fn2_capi.lib()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert hasattr(lib, n), n
        assert n in fn2_capi.EXPORTS, n
    assert lib.fn2_abi_version() == 3
    assert re.search(r"#define\s+FN2_ABI_VERSION\s+3\b", hdr)


@pytest.mark.parametrize("name", ["cat", "cat_bwd", "norm", "norm_bwd"])
def test_rejected_calls_return_codes_without_gpu(name):
    call, n = _calls(fn2_capi.lib())[name]
    good = [P] * 4
    for dt in (F16, BF16):
        for bad in (fn2_capi.FN2_F32, fn2_capi.FN2_F64, 7):
            assert call(good, bad, 20.0, 1, 3, 8, 8) == EDTYPE, bad
        assert call(good, dt, 20.0, 1, 0, 8, 8) == EINVAL               # C < 1
        assert call(good, dt, 20.0, 1, -2, 8, 8) == EINVAL
        assert call(good, dt, 20.0, -1, 3, 8, 8) == EINVAL              # B < 0
        assert call(good, dt, 20.0, 1, 3, 0, 8) == EINVAL               # H < 1
        for i in range(n):                                              # every tensor: NULL, then odd address
            p = list(good); p[i] = NULL
            assert call(p, dt, 20.0, 1, 3, 8, 8) == EINVAL, i
            p[i] = ODD
            assert call(p, dt, 20.0, 1, 3, 8, 8) == EALIGN, i
        assert call([NULL] * 4, dt, 20.0, 0, 3, 8, 8) == OK             # empty batch: nothing to do, nothing looked at
        if name.startswith("cat"):
            assert call(good, dt, 0.0, 1, 3, 8, 8) == EINVAL            # div_flow 0
            assert call(good, dt, float("nan"), 1, 3, 8, 8) == EINVAL   # div_flow NaN
