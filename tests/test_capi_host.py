"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/flownet2_hip.h declares, rejects bad calls before touching the GPU, and the pybind
modules / Python wrappers keep the reference's names and fail loudly without a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

import fn2_capi


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(fn2_[a-z0-9_]+)\s*\(", hdr)))


def test_header_symbols_exported():
    lib = fn2_capi.lib()
    names = declared_symbols()
    assert len(names) >= 11
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/flownet2_hip.h but not exported"
    assert sorted(fn2_capi.EXPORTS) == names
    assert lib.fn2_abi_version() == 3


def test_product_library_exports_only_the_public_abi():
    """The profiling entry points (csrc/fn2_debug.h) -- among them the one that sets a process-global timeline buffer -- live in
    libflownet2_hip_debug.so; the product library exports exactly the fn2_* symbols include/flownet2_hip.h declares
    ('no global mutable state')."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", fn2_capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3})
    # literally: no mangled fn2::... helpers, no kernel handles (-fvisibility=hidden + csrc/exports.map)
    assert exported == declared_symbols(), set(exported) ^ set(declared_symbols())
    dbg = fn2_capi.debug_lib()
    for n in fn2_capi.DEBUG_EXPORTS + fn2_capi.EXPORTS:
        assert hasattr(dbg, n), n


def test_output_shape_matches_reference_formula():
    # correlation_cuda.cc:19-34
    assert fn2_capi.correlation_output_shape(48, 64, 20, 1, 20, 1, 2) == (441, 48, 64)
    assert fn2_capi.correlation_output_shape(48, 64, 3, 3, 20, 1, 2) == (441, 12, 28)
    assert fn2_capi.correlation_output_shape(16, 16, 4, 1, 4, 2, 2) == (25, 8, 8)
    with pytest.raises(RuntimeError):
        fn2_capi.correlation_output_shape(4, 4, 0, 1, 20, 1, 2)   # empty output
    from oracle.oracle import corr_shapes
    for args in [(48, 64, 20, 1, 20, 1, 2), (10, 12, 2, 1, 4, 1, 2), (9, 9, 3, 3, 2, 2, 1), (17, 5, 4, 1, 4, 3, 2)]:
        assert fn2_capi.correlation_output_shape(*args) == corr_shapes(*args)[2:]


def test_rejected_calls_return_codes_without_gpu():
    lib = fn2_capi.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fn2_channelnorm_forward(p, p, 7, 1, 1, 2, 2, null) == -2            # FN2_EDTYPE
    assert lib.fn2_channelnorm_forward(p, p, 0, 1, 0, 2, 2, null) == -1            # C < 1
    assert lib.fn2_channelnorm_forward(null, p, 0, 1, 1, 2, 2, null) == -1         # null pointer
    assert lib.fn2_channelnorm_forward(p, p, 0, 0, 3, 2, 2, null) == 0             # empty batch: nothing to do
    assert lib.fn2_resample2d_forward(p, null, p, p, 1, 1, 2, 2, 2, 2, 0, 1, null) == -1   # kernel_size < 1: FN2_EINVAL
    assert lib.fn2_correlation_forward(p, p, p, 0, 1, 4, 4, 4, 0, 1, 20, 1, 2, null) == -1  # empty output
    assert lib.fn2_correlation_backward(p, p, p, p, p, 0, 1, 4, 8, 8, 4, 1, 4, 2, 2, null) == -4  # stride1 != 1
    assert lib.fn2_correlation_forward_ex(p, p, p, 0, 1, 4, 8, 8, 4, 3, 4, 1, 2, 2, null) == -4   # MFMA path needs k=1
    i64, f32 = ctypes.c_int64, ctypes.c_float
    assert lib.fn2_correlation_forward_fused(p, p, p, i64(10), f32(0.1), 0, 1, 4, 8, 8, 4, 1, 4, 1, 2, 0, null) == -1  # stride < 25*8*8
    assert lib.fn2_correlation_forward_fused(p, p, p, i64(3200), f32(0.1), 0, 0, 4, 8, 8, 4, 1, 4, 1, 2, 0, null) == 0   # empty batch
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    assert lib.fn2_channelnorm_forward(mis, p, 0, 1, 1, 2, 2, null) == -3          # FN2_EALIGN
    assert b"dtype" in lib.fn2_strerror(-2) and lib.fn2_strerror(0) == b"ok"
    # ABI v2 entry points (round 5): fn2_warp_diff_norm_cat_backward, fn2_multiscale_loss
    wb = lib.fn2_warp_diff_norm_cat_backward
    assert wb(p, p, p, p, null, p, f32(20.0), 1, 0, 8, 8, 1, null) == -1           # C < 1
    assert wb(p, p, p, p, null, p, f32(0.0), 1, 3, 8, 8, 1, null) == -1            # div_flow == 0
    assert wb(p, p, p, p, null, p, f32(float("nan")), 1, 3, 8, 8, 1, null) == -1   # div_flow nan
    assert wb(p, p, p, null, null, p, f32(20.0), 1, 3, 8, 8, 1, null) == -1        # no concat gradient
    assert wb(p, p, p, p, null, null, f32(20.0), 1, 3, 8, 8, 1, null) == -1        # no flow gradient to write
    assert wb(p, p, p, p, null, p, f32(20.0), 0, 3, 8, 8, 1, null) == 0            # empty batch
    assert wb(mis, p, p, p, null, p, f32(20.0), 1, 3, 8, 8, 1, null) == -3         # FN2_EALIGN
    assert lib.fn2_warp_diff_norm(p, p, null, 1, 3, 8, 8, 1, null) == -1                    # no output
    assert lib.fn2_warp_diff_norm(p, p, p, 1, 0, 8, 8, 1, null) == -1                       # C < 1
    assert lib.fn2_warp_diff_norm(p, p, p, 0, 3, 8, 8, 1, null) == 0                        # empty batch
    assert lib.fn2_warp_diff_norm_backward(p, p, p, null, p, 1, 3, 8, 8, 1, null) == -1     # no gradient of the norm
    assert lib.fn2_warp_diff_norm_backward(p, p, mis, p, p, 1, 3, 8, 8, 1, null) == -3      # FN2_EALIGN
    outs = (ctypes.c_void_p * 1)(p.value)
    w1 = (ctypes.c_float * 1)(0.32)
    ml = lib.fn2_multiscale_loss
    assert ml(outs, p, p, None, w1, f32(1.0), 3, 1, 8, 8, 4, 1, f32(0.05), p, ctypes.c_size_t(1 << 20), null) == -1    # norm must be 1 or 2
    assert ml(outs, p, p, None, w1, f32(1.0), 2, 1, 8, 8, 3, 1, f32(0.05), p, ctypes.c_size_t(1 << 20), null) == -1    # start_scale not a power of two
    assert ml(outs, p, p, None, w1, f32(1.0), 2, 1, 8, 8, 4, 1, f32(0.05), p, ctypes.c_size_t(0), null) == -1          # workspace too small
    for what, rc, want in rejected_correlation_calls(lib, fn2_capi.debug_lib()):
        assert rc == want, what


def rejected_correlation_calls(lib, dbg):
    """(what, code, expected code) of the correlation dispatcher's calls that end before any launch: every case of
    tests/corr_dispatch_cases.py whose plan is a code, through the entry point the plan speaks of -- fn2_correlation_forward_ex /
    _backward_ex, fn2_correlation_backward_fused as well (identity activation on a contiguous gradient: no mask pass in front of
    the dispatcher) and the debug entry points for a variant -- and the one rejection a plan cannot see, a launcher's own alignment
    check.  The expected codes are those of the if-chains the kernel table replaced.  Addresses are never dereferenced."""
    import corr_dispatch_cases as cases
    i64, f32, null = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p(0)
    for what, direction, dtype, shape, params, kw, want in cases.FORWARD_AUTO + cases.FORWARD_FORCED + cases.BACKWARD_AUTO + cases.DEBUG:
        if not isinstance(want, int):
            continue
        algo = kw.get("algo", fn2_capi.FN2_CORR_AUTO)
        ptrs = [ctypes.c_void_p(a) for a in kw.get("ptrs", (cases.A16,) * 5)]
        tail = (dtype,) + shape + params + (algo, null)
        if direction == "forward":
            fn = dbg.fn2_debug_correlation_forward if algo >= 100 else lib.fn2_correlation_forward_ex
            yield what, fn(*ptrs[:3], *tail), want
        else:
            fn = dbg.fn2_debug_correlation_backward if algo >= 100 else lib.fn2_correlation_backward_ex
            yield what, fn(*ptrs, *tail), want
    a16 = ctypes.c_void_p(cases.A16)
    yield "bwd stride1 2 (fused)", lib.fn2_correlation_backward_fused(a16, a16, a16, i64(1 << 20), a16, i64(1 << 20), f32(0.1), a16, ctypes.c_size_t(1 << 40),
                                                                      a16, a16, cases.F32, 1, 4, 8, 8, 4, 1, 4, 2, 2, 0, null), cases.EUNSUPPORTED
    for algo, want in ((5, cases.EINVAL), (-1, cases.EINVAL), (fn2_capi.FN2_CORR_MFMA_F16X2, cases.EUNSUPPORTED)):   # on (1, 16, 2, 2), md 4
        tail = (cases.F32,) + cases.SMALL + cases.md(4) + (algo, null)
        yield "bwd algo %d" % algo, lib.fn2_correlation_backward_ex(a16, a16, a16, a16, a16, *tail), want
        yield "bwd algo %d (fused)" % algo, lib.fn2_correlation_backward_fused(a16, a16, a16, i64(25 * 2 * 2), a16, i64(25 * 2 * 2), f32(1.0), a16,
                                                                              ctypes.c_size_t(1 << 40), a16, a16, *tail), want
    yield "half, forced f16x2, in1 off by 2 bytes", lib.fn2_correlation_forward_ex(
        ctypes.c_void_p(cases.A16 + 2), a16, a16, cases.HALF, 1, 128, 2, 8, *cases.P20, fn2_capi.FN2_CORR_MFMA_F16X2, null), cases.EALIGN


def test_float32_warp_entry_points_check_in_a_fixed_order():
    """Calls in which two checks of a float32 warp entry point disagree: dims and kernel_size (with div_flow) first, then empty -> FN2_OK,
    null -> FN2_EINVAL, (det) workspace -> FN2_EINVAL, alignment -> FN2_EALIGN.  Every call returns before any launch."""
    lib = fn2_capi.lib()
    OK, EINVAL, EALIGN = 0, -1, -3
    f32, sz = ctypes.c_float, ctypes.c_size_t
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p, mis = ctypes.c_void_p(base), ctypes.c_void_p(base + 2)
    ws, ws_mis = ctypes.c_void_p(base + 1024), ctypes.c_void_p(base + 1024 + 4)   # 8-byte aligned / only 4-byte aligned
    nan = f32(float("nan"))

    def dims(B, ks=None):   # B x 1 x 2 x 2, image of the flow's size
        return (B, 1, 2, 2, 2, 2) + (() if ks is None else (ks,))

    def pdims(B):           # the pair entry points: B, C, H, W
        return (B, 1, 2, 2)

    need = lib.fn2_resample2d_backward_det_workspace_bytes(*dims(1, 1))
    pneed = lib.fn2_warp_diff_norm_cat_backward_det_workspace_bytes(*pdims(1))
    assert 0 < need <= 1024 and 0 < pneed <= 1024
    fwd, bwd, bdet = lib.fn2_resample2d_forward, lib.fn2_resample2d_backward, lib.fn2_resample2d_backward_det
    cat, cbwd, cdet = lib.fn2_warp_diff_norm_cat, lib.fn2_warp_diff_norm_cat_backward, lib.fn2_warp_diff_norm_cat_backward_det
    nrm, nbwd = lib.fn2_warp_diff_norm, lib.fn2_warp_diff_norm_backward
    d20 = f32(20.0)
    table = [
        # B = 0 with null pointers: the empty check comes before the null check
        ("fwd empty", fwd, (null, null, null, null) + dims(0, 1) + (1, null), OK),
        ("bwd empty", bwd, (null, null, null, null, null, null) + dims(0, 1) + (1, null), OK),
        ("bdet empty", bdet, (null, null, null, null, null, null) + dims(0, 1) + (1, null, sz(0), null), OK),
        ("cat empty", cat, (null, null, null, d20) + pdims(0) + (1, null), OK),
        ("cbwd empty", cbwd, (null, null, null, null, null, null, d20) + pdims(0) + (1, null), OK),
        ("cdet empty", cdet, (null, null, null, null, null, null, d20) + pdims(0) + (1, null, sz(0), null), OK),
        ("nrm empty", nrm, (null, null, null) + pdims(0) + (1, null), OK),
        ("nbwd empty", nbwd, (null, null, null, null, null) + pdims(0) + (1, null), OK),
        # B = 0 with kernel_size = 0: kernel_size comes before the empty check
        ("fwd empty ks", fwd, (p, null, p, p) + dims(0, 0) + (1, null), EINVAL),
        ("bwd empty ks", bwd, (p, null, p, p, p, p) + dims(0, 0) + (1, null), EINVAL),
        ("bdet empty ks", bdet, (p, null, p, p, p, p) + dims(0, 0) + (1, ws, sz(1024), null), EINVAL),
        # div_flow = NaN with B = 0: div_flow is checked with the dims
        ("cat empty nan", cat, (p, p, p, nan) + pdims(0) + (1, null), EINVAL),
        ("cbwd empty nan", cbwd, (p, p, p, p, p, p, nan) + pdims(0) + (1, null), EINVAL),
        ("cdet empty nan", cdet, (p, p, p, p, p, p, nan) + pdims(0) + (1, ws, sz(1024), null), EINVAL),
        # a null pointer together with a misaligned one: null comes before alignment
        ("fwd null mis", fwd, (mis, null, p, null) + dims(1, 1) + (1, null), EINVAL),
        ("bwd null mis", bwd, (mis, null, p, p, p, null) + dims(1, 1) + (1, null), EINVAL),
        ("bdet null mis", bdet, (mis, null, p, p, p, null) + dims(1, 1) + (1, ws, sz(1024), null), EINVAL),
        ("cat null mis", cat, (mis, p, null, d20) + pdims(1) + (1, null), EINVAL),
        ("cbwd null mis", cbwd, (mis, p, p, p, p, null, d20) + pdims(1) + (1, null), EINVAL),
        ("cdet null mis", cdet, (mis, p, p, p, p, null, d20) + pdims(1) + (1, ws, sz(1024), null), EINVAL),
        ("nrm null mis", nrm, (mis, p, null) + pdims(1) + (1, null), EINVAL),
        ("nbwd null mis", nbwd, (mis, p, p, p, null) + pdims(1) + (1, null), EINVAL),
        # det: a workspace that is too small together with a misaligned pointer: the workspace comes before alignment
        ("bdet small ws mis", bdet, (mis, null, p, p, p, p) + dims(1, 1) + (1, ws, sz(need - 1), null), EINVAL),
        ("cdet small ws mis", cdet, (mis, p, p, p, p, p, d20) + pdims(1) + (1, ws, sz(pneed - 1), null), EINVAL),
        ("bdet no ws mis", bdet, (mis, null, p, p, p, p) + dims(1, 1) + (1, null, sz(1024), null), EINVAL),
        ("cdet no ws mis", cdet, (mis, p, p, p, p, p, d20) + pdims(1) + (1, null, sz(1024), null), EINVAL),
        # det: a misaligned workspace of sufficient size
        ("bdet ws mis", bdet, (p, null, p, p, p, p) + dims(1, 1) + (1, ws_mis, sz(1024), null), EALIGN),
        ("cdet ws mis", cdet, (p, p, p, p, p, p, d20) + pdims(1) + (1, ws_mis, sz(1024), null), EALIGN),
        # the concat row's det call without a pair gradient hands over to the atomic entry point only after its own workspace check
        ("cdet no grad_pair small ws", cdet, (p, p, p, p, null, p, d20) + pdims(1) + (1, ws, sz(pneed - 1), null), EINVAL),
        ("cdet no grad_pair no ws", cdet, (p, p, p, p, null, p, d20) + pdims(1) + (1, null, sz(1024), null), EINVAL),
        ("cdet no grad_pair ws mis", cdet, (p, p, p, p, null, p, d20) + pdims(1) + (1, ws_mis, sz(1024), null), EALIGN),
    ]
    for what, fn, args, want in table:
        assert fn(*args) == want, what


def test_modules_keep_reference_names_and_signatures():
    import channelnorm_cuda
    import correlation_cuda
    import resample2d_cuda
    for m in (correlation_cuda, resample2d_cuda, channelnorm_cuda):
        assert callable(m.forward) and callable(m.backward)
        assert ".so" in m.__file__ and os.path.dirname(m.__file__).endswith("flownet2-pytorch_amd")
    from networks.channelnorm_package.channelnorm import ChannelNorm, ChannelNormFunction
    from networks.correlation_package.correlation import Correlation, CorrelationFunction
    from networks.resample2d_package.resample2d import Resample2d, Resample2dFunction
    assert list(inspect.signature(Correlation.__init__).parameters)[1:] == [
        "pad_size", "kernel_size", "max_displacement", "stride1", "stride2", "corr_multiply"]
    assert [p.default for p in list(inspect.signature(Correlation.__init__).parameters.values())[1:]] == [0, 0, 0, 1, 2, 1]
    assert [p.default for p in list(inspect.signature(CorrelationFunction.forward).parameters.values())[3:]] == [3, 3, 20, 1, 2, 1]
    assert [p.default for p in list(inspect.signature(Resample2d.__init__).parameters.values())[1:]] == [1, True]
    assert [p.default for p in list(inspect.signature(ChannelNorm.__init__).parameters.values())[1:]] == [2]
    assert issubclass(Resample2dFunction, torch.autograd.Function) and issubclass(ChannelNormFunction, torch.autograd.Function)


def test_cpu_tensors_fail_loudly():
    """There is no CPU path behind the boundary: a CPU tensor must raise, not silently compute."""
    import channelnorm_cuda
    import correlation_cuda
    import resample2d_cuda
    a = torch.zeros(1, 16, 8, 8)
    e = torch.zeros(0)
    with pytest.raises(RuntimeError, match="GPU"):
        correlation_cuda.forward(a, a, e, e, e, 4, 1, 4, 1, 2, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        correlation_cuda.backward(a, a, e, e, a, e, e, 4, 1, 4, 1, 2, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        resample2d_cuda.forward(a, torch.zeros(1, 2, 8, 8), a.clone(), 1, True)
    with pytest.raises(RuntimeError, match="GPU"):
        channelnorm_cuda.forward(a, torch.zeros(1, 1, 8, 8), 2)
    with pytest.raises(TypeError):
        correlation_cuda.forward(a, a)   # positional signature of the reference binding


def test_product_path_never_imports_oracle():
    """oracle/ is test infrastructure: nothing under flownet2-pytorch_amd/ may reference it."""
    pkg = os.path.join(ROOT, "flownet2-pytorch_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h")):
                txt = open(os.path.join(d, f), errors="ignore").read()
                for needle in ("import oracle", "from oracle", "libfn2_oracle", "libfn2_ref", "fn2o_", "fn2ref_",
                               "oracle/", "oracle.py"):
                    assert needle not in txt, (os.path.join(d, f), needle)
