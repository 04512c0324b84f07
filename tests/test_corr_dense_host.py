"""CPU-side checks of the dense stride-1 correlation kernels' handle (csrc/correlation_dense.hip): the debug variant that names
them is declared where the header documents it, and no public selector, C symbol or ABI version came with them.  Every call
here returns in front of a launch (empty batch, misaligned pointer, bad parameter): there is no GPU to launch on."""
import ctypes
import os
import re
import subprocess

from conftest import PKG, ROOT

import fn2_capi

EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4
DENSE = (4, 1, 4, 1, 1)   # pad_size, kernel_size, max_displacement, stride1, stride2


def test_dense_debug_variant_declared():
    hdr = open(os.path.join(PKG, "csrc", "fn2_debug.h")).read()
    m = re.search(r"#define\s+FN2_DEBUG_CORR_DENSE\s+(\d+)", hdr)
    assert fn2_capi.FN2_DEBUG_CORR_DENSE == int(m.group(1))
    assert re.search(r"//\s+both\s+:\s+%d\b" % fn2_capi.FN2_DEBUG_CORR_DENSE, hdr), "the variant table names the value"
    # outside the documented profiling ranges: forward 100 .. 4999 and 5000 + v (switch bits below 128), backward 100 + v; it is
    # routed to the debug entry points (algo >= 100)
    v = fn2_capi.FN2_DEBUG_CORR_DENSE
    assert v >= 100 and not 100 <= v <= 4999 and not 5000 <= v < 5128 and not 6000 <= v < 6128


def test_dense_adds_no_public_selector_symbol_or_abi():
    lib = fn2_capi.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    i64, f32 = ctypes.c_int64, ctypes.c_float
    for dt in (0, 1, 3):
        for algo in (5, 99, fn2_capi.FN2_DEBUG_CORR_DENSE):   # the public entry points know none of them
            assert lib.fn2_correlation_forward_ex(p, p, p, dt, 1, 4, 8, 8, *DENSE, algo, null) == EINVAL
            assert lib.fn2_correlation_backward_ex(p, p, p, p, p, dt, 1, 4, 8, 8, *DENSE, algo, null) == EINVAL
            assert lib.fn2_correlation_forward_fused(p, p, p, i64(81 * 64), f32(0.1), dt, 1, 4, 8, 8, *DENSE, algo, null) == EINVAL
        # the dense configuration at the public entry points: the usual checks, in front of any launch
        assert lib.fn2_correlation_forward_ex(p, p, p, dt, 0, 4, 8, 8, *DENSE, 0, null) == 0            # empty batch
        assert lib.fn2_correlation_backward_ex(p, p, p, p, p, dt, 0, 4, 8, 8, *DENSE, 0, null) == 0
        assert lib.fn2_correlation_forward_ex(mis, p, p, dt, 1, 4, 8, 8, *DENSE, 0, null) == EALIGN
        assert lib.fn2_correlation_backward_ex(p, p, p, p, mis, dt, 1, 4, 8, 8, *DENSE, 0, null) == EALIGN
        assert lib.fn2_correlation_forward_fused(p, p, p, i64(10), f32(0.1), dt, 1, 4, 8, 8, *DENSE, 0, null) == EINVAL   # slice too small
    assert lib.fn2_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(fn2_capi.EXPORTS) == sorted(set(re.findall(r"\b(fn2_[a-z0-9_]+)\s*\(", code)))
    assert len(fn2_capi.EXPORTS) == 31
    assert "FN2_DEBUG_CORR_DENSE" not in code, "the debug variant is no part of the public header's declarations"


def test_dense_debug_entry_points_check_before_launch():
    dbg = fn2_capi.debug_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    V = fn2_capi.FN2_DEBUG_CORR_DENSE
    fwd, bwd = dbg.fn2_debug_correlation_forward, dbg.fn2_debug_correlation_backward
    assert fwd(p, p, p, 0, 0, 4, 8, 8, *DENSE, V, null) == 0                       # empty batch
    assert bwd(p, p, p, p, p, 0, 0, 4, 8, 8, *DENSE, V, null) == 0
    assert fwd(mis, p, p, 0, 1, 4, 8, 8, *DENSE, V, null) == EALIGN
    assert bwd(p, p, p, p, mis, 3, 1, 4, 8, 8, *DENSE, V, null) == EALIGN
    assert fwd(p, p, p, 7, 1, 4, 8, 8, *DENSE, V, null) == EDTYPE
    # outside the domain: declined, nothing launched (there is no GPU here to launch on)
    for params, dt in (((20, 1, 20, 1, 2), 0), ((3, 3, 4, 1, 1), 0), ((4, 1, 4, 2, 1), 0), ((2, 1, 4, 1, 1), 0), ((5, 1, 5, 1, 1), 0),
                       (DENSE, 2)):
        assert fwd(p, p, p, dt, 1, 4, 16, 16, *params, V, null) == EUNSUPPORTED, params
        assert bwd(p, p, p, p, p, dt, 1, 4, 16, 16, *params, V, null) == EUNSUPPORTED, params


def test_dense_kernels_use_no_scratch(tmp_path):
    """The backward's inner loop is shaped (scheduling groups, an anchor for the sums, a packed multiply written by hand) so that
    the compiler keeps everything in registers; DESIGN.md 4.9 records 0 bytes of scratch for all 24 instantiations.  A compiler
    that brings the spills back fails here, not silently in a benchmark.  Device code only, the library's own flags."""
    import build
    src = os.path.join(PKG, "csrc", "correlation_dense.hip")
    r = subprocess.run([build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "dense.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S*corr_(?:fwd|bwd)_dense\S*)(.*?)LDS Size", r.stderr, flags=re.S)
    assert len(kernels) == 24, [k for k, _ in kernels]
    for name, body in kernels:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
        assert scratch == 0, f"{name} spills {scratch} bytes per lane"
