"""CPU-side checks of CorrLookup's library (include/flownet2_hip_lookup.h, libflownet2_hip_lookup.so; what it exports and
links is in tests/test_libraries_host.py): the three headers in one translation unit, every rejection in front of a launch (host pointers, no GPU), the float64 reference
against RAFT's all-pairs + grid_sample composition (values and both gradients), and the staged kernels' register budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import corr_lookup_ref as RL
import fn2_capi

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
STAGED_KERNELS = 10   # forward and grad_fmap1, r = 0 .. 4

# (H, W, H2, W2, r, C)
GEOMETRIES = [(5, 6, 5, 6, 2, 3), (4, 7, 2, 3, 1, 5), (3, 4, 3, 4, 0, 2), (4, 5, 2, 2, 4, 4)]


def test_three_headers_in_one_translation_unit(tmp_path):
    """The lookup header restates the codes unless one of the other two came first."""
    for i, incs in enumerate((("flownet2_hip.h", "flownet2_hip_ext.h", "flownet2_hip_lookup.h"), ("flownet2_hip_ext.h", "flownet2_hip_lookup.h"),
                              ("flownet2_hip.h", "flownet2_hip_lookup.h"), ("flownet2_hip_lookup.h",))):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in incs) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2L_LOOKUP_STAGED + FN2L_MAX_RADIUS];\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.lookup_lib()
    fwd, bwd = lib.fn2l_corr_lookup_forward, lib.fn2l_corr_lookup_backward
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    sc = ctypes.c_float(0.25)
    shape = (1, 4, 8, 16, 4, 8)   # B, C, H, W, H2, W2

    def f(ptrs, dt, shp, r, algo):
        return fwd(*ptrs, dt, *shp, r, sc, algo, null)

    def b(ptrs, dt, shp, r, algo):
        return bwd(*ptrs, dt, *shp, r, sc, algo, null)

    for call, n in ((f, 4), (b, 6)):
        good = [p] * n
        # dtype first of all: anything but float32, whatever else is wrong
        for dt in (1, 2, 3, 7, -1):
            assert call([null] * n, dt, (1, 0, 8, 16, 4, 8), 9, 5) == EDTYPE, dt
        # radius, then the sizes
        for r in (-1, 9, 100):
            assert call([null] * n, 0, (1, 0, 8, 16, 4, 8), r, 5) == EINVAL, r
        for shp in ((1, 0, 8, 16, 4, 8), (1, 4, 0, 16, 4, 8), (1, 4, 8, 0, 4, 8), (1, 4, 8, 16, 0, 8), (1, 4, 8, 16, 4, 0), (-1, 4, 8, 16, 4, 8),
                    (1, -4, 8, 16, 4, 8), (1, 4, 8, 16, -4, 8)):
            assert call([null] * n, 0, shp, 4, 5) == EINVAL, shp
        # a plane beyond 32-bit indices
        assert call([null] * n, 0, (1, 1, 65536, 32768, 4, 8), 4, 0) == EUNSUPPORTED
        assert call([null] * n, 0, (1, 1, 4, 8, 65536, 32768), 4, 0) == EUNSUPPORTED
        # empty batch: nothing to do, whatever the pointers and the selector
        for algo in (0, 1, 2, 77):
            assert call([null] * n, 0, (0,) + shape[1:], 4, algo) == OK
        # NULL pointers, also next to a misaligned one and a bad selector: NULL is reported first
        for i in range(n):
            ptrs = list(good)
            ptrs[i] = null
            ptrs[(i + 1) % n] = mis
            assert call(ptrs, 0, shape, 4, 9) == EINVAL, i
        # alignment to 4 bytes, before the selector
        for i in range(n):
            ptrs = list(good)
            ptrs[i] = mis
            assert call(ptrs, 0, shape, 5, 2) == EALIGN, i
        # unknown selectors, before the staged domain
        for algo in (-1, 3, 4, 9000):
            assert call(good, 0, shape, 5, algo) == EINVAL, algo
        # FN2L_LOOKUP_STAGED outside its domain: r = 5 .. 8
        for r in range(RL.header_macros()["FN2L_STAGED_MAX_RADIUS"] + 1, 9):
            assert call(good, 0, shape, r, 2) == EUNSUPPORTED, r
    with pytest.raises(RuntimeError):
        fn2_capi.check(EUNSUPPORTED, "fn2l_corr_lookup_forward")


def test_cpu_tensors_and_bad_arguments_are_refused():
    import corr_lookup_cuda
    from networks.correlation_package import AlternateCorrBlock, CorrLookup, CorrLookupFunction
    a, b, c = torch.zeros(1, 4, 8, 16), torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 8, 16)
    e = torch.zeros(0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_lookup_cuda.forward(a, b, c, e, 2, 0.5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_lookup_cuda.backward(a, b, c, torch.zeros(1, 25, 8, 16), e, e.clone(), 2, 0.5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_lookup_cuda.forward_alloc(a, b, c, 2, 0.5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        CorrLookupFunction.apply(a, b, c, 2, 0.5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        CorrLookup(2)(a, b, c)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        AlternateCorrBlock(a, b, num_levels=2, radius=2)(c)
    with pytest.raises(RuntimeError, match="detach"):   # before anything else: a silent None would train wrongly
        CorrLookupFunction.apply(a, b, c.clone().requires_grad_(True), 2, 0.5)
    m = CorrLookup(3)
    assert (m.radius, m.scale) == (3, None) and "radius=3" in repr(m)


def test_reference_decodes_coordinates_as_the_header_says():
    c = np.zeros((1, 2, 1, 8), np.float32)
    c[0, 0, 0] = [2.0, -0.25, -1e-10, 3.75, np.nan, np.inf, 2.0 ** 20, -(2.0 ** 20) + 0.125]
    c[0, 1, 0] = [0.5, -3.0, 7.0, -1e30, 0.0, 0.0, 0.0, 0.0]
    x0, y0, fx, fy, ok = RL.decode(c)
    assert ok[0, 0].tolist() == [True, True, True, False, False, False, False, True]
    assert x0[0, 0, :3].tolist() == [2, -1, -1] and fx[0, 0, :3].tolist() == [0.0, 0.75, 1.0]   # floor, not truncation; fl32(1 - 1e-10) = 1
    assert y0[0, 0, :3].tolist() == [0, -3, 7] and fy[0, 0, :3].tolist() == [0.5, 0.0, 0.0]
    assert x0[0, 0, 7] == -(2 ** 20) and fx[0, 0, 7] == 0.125


def _case(geo, seed):
    """Inputs of one geometry: coordinates from -2.5 to size + 1.5 on a 2^-10 lattice (so that fl32(c - floor(c)) is exact and the
    composition, which sees the coordinates as float64 numbers, is the same function), one integer and one negative fractional
    coordinate pinned."""
    H, W, H2, W2, r, C = geo
    rng = np.random.default_rng(seed)
    f1 = rng.standard_normal((2, C, H, W))
    f2 = rng.standard_normal((2, C, H2, W2))
    co = np.stack([rng.uniform(-2.5, W2 + 1.5, (2, H, W)), rng.uniform(-2.5, H2 + 1.5, (2, H, W))], 1)
    co = np.round(co * 1024) / 1024
    co[0, :, 0, 0] = (1.0, 0.0)          # integer coordinates: both fractions 0, the weight-0 taps are terms
    co[1, :, 1, 1] = (-0.25, -1.75)      # negative fractions: floor, not truncation
    return f1, f2, co.astype(np.float32), float(C) ** -0.5


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
def test_reference_forward_is_rafts_composition(geo):
    f1, f2, co, scale = _case(geo, seed=sum(geo))
    r = geo[4]
    ref, S = RL.forward(f1, f2, co, r, scale)
    got = RL.compose(torch.from_numpy(f1), torch.from_numpy(f2), torch.from_numpy(co).double(), r, scale).numpy()
    assert ref.shape == got.shape == (2, (2 * r + 1) ** 2, geo[0], geo[1])
    assert np.abs(ref - got).max() < 1e-12, float(np.abs(ref - got).max())
    assert np.abs(ref).max() > 0.1 and (S >= np.abs(ref) - 1e-12).all()


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
def test_reference_gradients_are_autograd_through_the_composition(geo):
    f1, f2, co, scale = _case(geo, seed=sum(geo) + 1)
    r = geo[4]
    go = np.random.default_rng(5).standard_normal((2, (2 * r + 1) ** 2, geo[0], geo[1]))
    (g1, S1), (g2, S2, n2) = RL.backward(f1, f2, co, go, r, scale)
    t1, t2 = torch.from_numpy(f1).requires_grad_(True), torch.from_numpy(f2).requires_grad_(True)
    RL.compose(t1, t2, torch.from_numpy(co).double(), r, scale).backward(torch.from_numpy(go))
    assert np.abs(g1 - t1.grad.numpy()).max() < 1e-10 and np.abs(g2 - t2.grad.numpy()).max() < 1e-10
    assert np.abs(g1).max() > 0.1 and np.abs(g2).max() > 0.1
    assert (g2[n2 == 0] == 0).all() and (S2[n2 == 0] == 0).all() and n2.max() >= 4


def test_reference_absent_taps_and_pixels_without_taps():
    """An inf outside the window's reach is harmless, a tap outside fmap2 is absent (not 0 * inf), a bad pixel gives zeros."""
    f1 = np.ones((1, 1, 1, 3))
    f2 = np.arange(1.0, 7.0).reshape(1, 1, 2, 3)
    co = np.array([[[[0.0, -100.0, np.nan]], [[0.0, 0.0, 0.0]]]], np.float32)
    ref, S = RL.forward(f1, f2, co, 1, 2.0)
    # pixel 0 at (0, 0): channel i * 3 + j is fmap2[j - 1, i - 1], absent for a negative index
    assert ref[0, :, 0, 0].tolist() == [0, 0, 0, 0, 2, 8, 0, 4, 10]
    assert (ref[0, :, 0, 1:] == 0).all() and (S[0, :, 0, 1:] == 0).all()
    (g1, _), (g2, _, n2) = RL.backward(f1, f2, co, np.ones((1, 9, 1, 3)), 1, 2.0)
    assert g1[0, 0, 0].tolist() == [2.0 * (1 + 2 + 4 + 5), 0, 0]
    assert g2[0, 0].tolist() == [[2, 2, 0], [2, 2, 0]] and n2[0, 0].tolist() == [[4, 4, 2], [4, 4, 2]]   # (a weight-0 tap inside is a term)


def test_staged_kernels_use_no_scratch(tmp_path):
    """0 bytes of scratch for every staged instantiation (DESIGN.md 4.11 records the budgets), and for the general kernels too;
    device code only, the library's own flags."""
    import build
    src = os.path.join(PKG, "csrc", "corr_lookup.hip")
    r = subprocess.run([build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "corr_lookup.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S*lookup_\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", r.stderr, flags=re.S)
    staged = [k for k in kernels if "staged" in k[0]]
    assert len(staged) == STAGED_KERNELS, [k for k, _, _ in kernels]
    assert len(kernels) == STAGED_KERNELS + 3 * 9   # general forward, grad_fmap1 and the scatter for r = 0 .. 8
    for name, body, lds in kernels:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
        assert scratch == 0, f"{name} spills {scratch} bytes per lane"
        assert int(lds) <= 60 * 1024, f"{name} uses {lds} bytes of LDS"
