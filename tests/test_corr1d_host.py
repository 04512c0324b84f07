"""CPU-side checks of Correlation1d's sibling library (include/flownet2_hip_ext.h, libflownet2_hip_ext.so; what it exports and
links is in tests/test_libraries_host.py): that the main library and its ABI are untouched, the shape function, every rejection in front of a launch (host pointers, no GPU),
the float64 reference against the 2-D oracle's centre row, and the tiled kernels' register budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import corr1d_ref as R1
import fn2_capi

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
TILED_KERNELS = 30   # forward: 6 wave counts x 3 types; backward: 4 factor brackets x 3 types


def test_main_library_untouched():
    assert fn2_capi.lib().fn2_abi_version() == 3
    assert len(fn2_capi.EXPORTS) == 31
    assert not any(n.startswith("fn2x_") for n in fn2_capi.EXPORTS + fn2_capi.DEBUG_EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    assert "fn2x_" not in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", fn2_capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "fn2x_" not in out and "corr1d" not in out


@pytest.mark.parametrize("args", [(48, 96, 40, 40, 1, 1, 0), (48, 96, 40, 40, 1, 1, 1), (48, 96, 40, 40, 1, 1, -1), (5, 19, 2, 5, 1, 1, 0),
                                  (7, 19, 5, 5, 2, 1, 0), (7, 20, 0, 3, 2, 2, -1), (9, 31, 6, 6, 1, 2, 1), (3, 11, 0, 0, 3, 1, 0)],
                         ids=lambda a: "-".join(map(str, a)))
def test_output_shape_matches_the_formula(args):
    H, W, pad, md, s1, s2, sd = args
    dr = md // s2
    want = (2 * dr + 1 if sd == 0 else dr + 1, -(-H // s1), -(-(W + 2 * pad - 2 * md) // s1))
    assert fn2_capi.correlation1d_output_shape(*args) == want == R1.out_shape(*args)


def test_output_shape_rejects():
    lib = fn2_capi.ext_lib()
    n = ctypes.c_int()
    r = ctypes.byref(n)
    assert lib.fn2x_correlation1d_output_shape(4, 8, 0, 4, 1, 1, 0, r, r, r) == EINVAL     # empty output: 8 - 8 columns
    assert lib.fn2x_correlation1d_output_shape(4, 8, 1, 5, 1, 1, 0, r, r, r) == EINVAL     # 8 + 2 - 10
    assert lib.fn2x_correlation1d_output_shape(4, 9, 0, 4, 1, 1, 0, r, r, r) == OK
    for bad in ((0, 8, 0, 0, 1, 1, 0), (4, 0, 0, 0, 1, 1, 0), (4, 8, -1, 0, 1, 1, 0), (4, 8, 0, -1, 1, 1, 0), (4, 8, 0, 0, 0, 1, 0),
                (4, 8, 0, 0, 1, 0, 0), (4, 8, 0, 0, 1, 1, 2), (4, 8, 0, 0, 1, 1, -2)):
        assert lib.fn2x_correlation1d_output_shape(*bad, r, r, r) == EINVAL, bad
    with pytest.raises(RuntimeError):
        fn2_capi.correlation1d_output_shape(4, 8, 0, 4, 1, 1, 0)


def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch: there is no GPU here to launch on, and the pointers are host memory."""
    lib = fn2_capi.ext_lib()
    fwd, bwd = lib.fn2x_correlation1d_forward, lib.fn2x_correlation1d_backward
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    ok = (4, 4, 1, 1, 0)   # pad_size, max_displacement, stride1, stride2, single_direction
    for dt in (0, 1, 2, 3):
        # bad shape / parameter
        for shape, prm in (((1, 0, 8, 16), ok), ((1, 4, 0, 16), ok), ((1, 4, 8, 0), ok), ((-1, 4, 8, 16), ok), ((1, 4, 8, 16), (-1, 4, 1, 1, 0)),
                           ((1, 4, 8, 16), (4, -1, 1, 1, 0)), ((1, 4, 8, 16), (4, 4, 0, 1, 0)), ((1, 4, 8, 16), (4, 4, 1, 0, 0)),
                           ((1, 4, 8, 16), (4, 4, 1, 1, 2)), ((1, 4, 8, 16), (4, 4, 1, 1, -2)), ((1, 4, 8, 8), (0, 4, 1, 1, 0))):
            assert fwd(p, p, p, dt, *shape, *prm, 0, null) == EINVAL, (shape, prm)
            assert bwd(p, p, p, p, p, dt, *shape, *prm, 0, null) == EINVAL, (shape, prm)
        # NULL pointers, also next to a misaligned one: NULL is reported before alignment
        assert fwd(null, p, p, dt, 1, 4, 8, 16, *ok, 0, null) == EINVAL
        assert fwd(p, null, p, dt, 1, 4, 8, 16, *ok, 0, null) == EINVAL
        assert fwd(mis, p, null, dt, 1, 4, 8, 16, *ok, 0, null) == EINVAL
        for i in range(5):
            ptrs = [p] * 5
            ptrs[i] = null
            ptrs[(i + 1) % 5] = mis
            assert bwd(*ptrs, dt, 1, 4, 8, 16, *ok, 0, null) == EINVAL, i
        # alignment to the element size
        for i in range(3):
            ptrs = [p] * 3
            ptrs[i] = mis
            assert fwd(*ptrs, dt, 1, 4, 8, 16, *ok, 0, null) == EALIGN, i
        for i in range(5):
            ptrs = [p] * 5
            ptrs[i] = mis
            assert bwd(*ptrs, dt, 1, 4, 8, 16, *ok, 0, null) == EALIGN, i
        # backward with stride1 != 1, before the pointers are looked at
        assert bwd(null, p, p, p, p, dt, 1, 4, 8, 16, 4, 4, 2, 1, 0, 0, null) == EUNSUPPORTED
        # empty batch: nothing to do, whatever the pointers
        for algo in (0, 1, 2):
            assert fwd(null, null, null, dt, 0, 4, 8, 16, *ok, algo, null) == OK
            assert bwd(null, null, null, null, null, dt, 0, 4, 8, 16, *ok, algo, null) == OK
        # unknown selectors
        for algo in (-1, 3, 4, 9000):
            assert fwd(p, p, p, dt, 1, 4, 8, 16, *ok, algo, null) == EINVAL, algo
            assert bwd(p, p, p, p, p, dt, 1, 4, 8, 16, *ok, algo, null) == EINVAL, algo
    # bad dtype: first of all
    assert fwd(null, null, null, 7, 1, 0, 8, 16, *ok, 0, null) == EDTYPE
    assert bwd(null, null, null, null, null, -1, 1, 0, 8, 16, 4, 4, 2, 1, 0, 0, null) == EDTYPE
    # FN2X_CORR1D_TILED outside the tiled domain, each reason: declined before any launch
    outside = [("stride2 = 2", 0, (1, 4, 8, 16), (4, 4, 1, 2, 0)), ("pad != md", 0, (1, 4, 8, 16), (3, 4, 1, 1, 0)),
               ("nOut = 83", 0, (1, 4, 8, 16), (41, 41, 1, 1, 0)), ("nOut = 82, one-sided", 1, (1, 4, 8, 16), (81, 81, 1, 1, 1)),
               ("double", 2, (1, 4, 8, 16), ok), ("stride1 = 2 (forward)", 3, (1, 4, 8, 16), (4, 4, 2, 1, 0)),
               ("beyond 32-bit offsets of one item", 0, (1, 2044, 1024, 1024), ok), ("beyond the grid's z extent", 1, (32768, 1, 1, 16), ok)]
    for why, dt, shape, prm in outside:
        assert fwd(p, p, p, dt, *shape, *prm, 2, null) == EUNSUPPORTED, why
        if prm[2] == 1:
            assert bwd(p, p, p, p, p, dt, *shape, *prm, 2, null) == EUNSUPPORTED, why


def test_cpu_tensors_are_refused():
    import correlation1d_cuda
    from networks.correlation_package import Correlation1d, Correlation1dFunction
    a = torch.zeros(1, 4, 8, 16)
    e = torch.zeros(0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        correlation1d_cuda.forward(a, a, e, 4, 4, 1, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        correlation1d_cuda.backward(a, a, torch.zeros(1, 9, 8, 16), e, e.clone(), 4, 4, 1, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        correlation1d_cuda.forward_alloc(a, a, 4, 4, 1, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        correlation1d_cuda.backward_alloc(a, a, torch.zeros(1, 9, 8, 16), 4, 4, 1, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        Correlation1dFunction.apply(a, a, 4, 4, 1, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        Correlation1d(4, 4)(a, a)
    m = Correlation1d()
    assert (m.pad_size, m.max_displacement, m.stride1, m.stride2, m.single_direction) == (0, 0, 1, 1, 0)


@pytest.mark.parametrize("case", [(4, 1, 1), (6, 1, 2), (5, 2, 1)], ids=lambda c: "md%d-s1_%d-s2_%d" % c)
def test_reference_is_the_centre_row_of_the_2d_oracle(oracle, case):
    """For pad == md the 1-D definition is the centre row of the 2-D layer's displacement window.  corr1d_ref is float64, the
    oracle fp32: the header's forward and backward bounds are the tolerance."""
    md, s1, s2 = case
    B, C, H, W = 2, 7, 5, 19
    rng = np.random.default_rng(100 + md)
    a = rng.standard_normal((B, C, H, W)).astype(np.float32)
    b = rng.standard_normal((B, C, H, W)).astype(np.float32)
    dr = md // s2
    D = 2 * dr + 1
    rows = slice(dr * D, (dr + 1) * D)
    full = oracle.corr_fwd(a, b, md, 1, md, s1, s2)
    ref, absr, bad = R1.forward(a, b, md, md, s1, s2, 0)
    assert not bad.any() and full[:, rows].shape == ref.shape
    err = np.abs(full[:, rows].astype(np.float64) - ref)
    assert (err <= R1.delta_fwd_f32(ref, absr, C)).all(), float((err / R1.delta_fwd_f32(ref, absr, C).clip(1e-300)).max())
    assert np.abs(ref).max() > 0.1
    # one-sided searches are the two halves of that row
    for sd, sl in ((-1, slice(0, dr + 1)), (1, slice(dr, D))):
        half, _, _ = R1.forward(a, b, md, md, s1, s2, sd)
        assert np.array_equal(half, ref[:, sl])
    if s1 != 1:
        return   # the backward is defined for stride1 = 1 only
    go = rng.standard_normal(ref.shape).astype(np.float32)
    go2d = np.zeros(full.shape, np.float32)
    go2d[:, rows] = go
    o1, o2 = oracle.corr_bwd(a, b, go2d, md, 1, md, s1, s2)
    (r1, ab1, n1), (r2, ab2, n2) = R1.backward(a, b, go, md, md, s1, s2, 0)
    assert not (n1.any() or n2.any())
    for got, r, ab in ((o1, r1, ab1), (o2, r2, ab2)):
        assert (np.abs(got.astype(np.float64) - r) <= R1.delta_bwd_f32(r, ab, D)).all()
        assert np.abs(r).max() > 0.1


def test_reference_absent_terms_and_nonfinite_masks():
    """pad < md: outputs start md - pad columns in; a term outside is absent, so an inf at the border poisons only the outputs
    that pair it with a pixel of the image."""
    a = np.ones((1, 1, 1, 6))
    b = np.arange(6, dtype=np.float64).reshape(1, 1, 1, 6)
    ref, absr, bad = R1.forward(a, b, 0, 2, 1, 1, 0)          # x1 = x + 2, x = 0, 1;  t = -2 .. 2
    assert ref.shape == (1, 5, 1, 2)
    assert np.array_equal(ref[0, :, 0, 0], [0, 1, 2, 3, 4]) and np.array_equal(ref[0, :, 0, 1], [1, 2, 3, 4, 5])
    b[0, 0, 0, 5] = np.inf
    ref, absr, bad = R1.forward(a, b, 2, 2, 1, 1, 0)          # pad == md: x1 = x
    assert bad.sum() == 3 and all(bad[0, o, 0, 5 - (o - 2)] for o in (2, 3, 4))   # x + t = 5 with x inside the image
    assert ref[0, 4, 0, 5] == 0 and not bad[0, 4, 0, 5]       # x + 2 = 7 is outside: absent


def test_tiled_kernels_use_no_scratch(tmp_path):
    """0 bytes of scratch for every tiled instantiation (DESIGN.md 4.10 records the budgets); a compiler that brings spills back
    fails here, not silently in a benchmark.  Device code only, the library's own flags."""
    import build
    src = os.path.join(PKG, "csrc", "correlation_1d.hip")
    r = subprocess.run([build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "corr1d.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S*corr1d_(?:fwd|bwd)_tiled\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", r.stderr, flags=re.S)
    assert len(kernels) == TILED_KERNELS, [k for k, _, _ in kernels]
    for name, body, lds in kernels:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
        assert scratch == 0, f"{name} spills {scratch} bytes per lane"
        assert int(lds) <= 32 * 1024, f"{name} uses {lds} bytes of LDS"
