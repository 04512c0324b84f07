"""CPU checks of the deterministic Resample2d / WarpDiffNormCat image gradient (fn2_*_backward_det): the C ABI declares and exports
the new entry points, sizes and rejects without a GPU, and the numpy restatement of the contract (tests/resample_det_ref.py) stays
within the documented error bound of the exact sum on adversarial planes."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import fn2_capi
import resample_det_ref as R

NEW = ["fn2_resample2d_backward_det_workspace_bytes", "fn2_resample2d_backward_det",
       "fn2_warp_diff_norm_cat_backward_det_workspace_bytes", "fn2_warp_diff_norm_cat_backward_det"]


def test_new_symbols_declared_exported_listed():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flownet2_hip.h")).read(), flags=re.S)
    lib = fn2_capi.lib()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert hasattr(lib, n), n
        assert n in fn2_capi.EXPORTS, n
    assert lib.fn2_resample2d_backward_det_workspace_bytes.restype is ctypes.c_size_t
    assert lib.fn2_warp_diff_norm_cat_backward_det_workspace_bytes.restype is ctypes.c_size_t
    assert lib.fn2_abi_version() == 3


@pytest.mark.parametrize("shape", [(8, 3, 384, 512, 384, 512, 1), (1, 1, 1, 1, 1, 1, 1), (2, 5, 20, 36, 24, 40, 3),
                                   (3, 64, 17, 30, 17, 30, 2), (0, 3, 8, 8, 8, 8, 1)])
def test_workspace_size_formula(shape):
    B, C, Hi, Wi, H, W, k = shape
    lib = fn2_capi.lib()
    planes = B * C
    want = (4 * planes + 255) // 256 * 256 + 8 * planes * Hi * Wi
    assert lib.fn2_resample2d_backward_det_workspace_bytes(B, C, Hi, Wi, H, W, k) == want
    if C >= 1 and Hi >= 1:
        assert lib.fn2_warp_diff_norm_cat_backward_det_workspace_bytes(B, C, Hi, Wi) == want
    assert lib.fn2_resample2d_backward_det_workspace_bytes(B, C, Hi, Wi, H, W, 0) == 0     # kernel_size < 1
    assert lib.fn2_warp_diff_norm_cat_backward_det_workspace_bytes(B, 0, Hi, Wi) == 0       # C < 1


def test_rejected_calls_return_codes_without_gpu():
    lib = fn2_capi.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    sz, f32 = ctypes.c_size_t, ctypes.c_float
    need = lib.fn2_resample2d_backward_det_workspace_bytes(1, 3, 8, 8, 8, 8, 1)
    rb = lib.fn2_resample2d_backward_det
    assert rb(p, null, p, p, p, p, 1, 3, 8, 8, 8, 8, 1, 1, null, sz(need), null) == -1          # NULL workspace
    assert rb(p, null, p, p, p, p, 1, 3, 8, 8, 8, 8, 1, 1, p, sz(need - 1), null) == -1         # short workspace
    assert rb(p, null, p, p, p, p, 1, 3, 8, 8, 8, 8, 0, 1, p, sz(need), null) == -1             # kernel_size < 1
    assert rb(p, null, p, p, null, p, 1, 3, 8, 8, 8, 8, 1, 1, p, sz(need), null) == -1          # no grad_img
    assert rb(p, null, p, p, p, p, 1, -1, 8, 8, 8, 8, 1, 1, p, sz(need), null) == -1            # C < 0
    assert rb(p, null, p, p, p, p, 0, 3, 8, 8, 8, 8, 1, 1, null, sz(0), null) == 0              # empty batch: nothing to do
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert rb(p, null, p, p, p, p, 1, 3, 8, 8, 8, 8, 1, 1, mis, sz(need), null) == -3           # workspace not 8-byte aligned
    needw = lib.fn2_warp_diff_norm_cat_backward_det_workspace_bytes(1, 3, 8, 8)
    wb = lib.fn2_warp_diff_norm_cat_backward_det
    assert wb(p, p, p, p, p, p, f32(20.0), 1, 3, 8, 8, 1, null, sz(needw), null) == -1          # NULL workspace
    assert wb(p, p, p, p, p, p, f32(20.0), 1, 3, 8, 8, 1, p, sz(needw - 8), null) == -1        # short workspace
    assert wb(p, p, p, p, null, p, f32(20.0), 1, 3, 8, 8, 1, null, sz(needw), null) == -1      # NULL workspace, no pair gradient too
    assert wb(p, p, p, p, p, p, f32(0.0), 1, 3, 8, 8, 1, p, sz(needw), null) == -1             # div_flow == 0
    assert wb(p, p, p, p, p, p, f32(20.0), 1, 0, 8, 8, 1, p, sz(needw), null) == -1            # C < 1
    assert wb(p, p, p, p, p, p, f32(20.0), 0, 3, 8, 8, 1, null, sz(0), null) == 0              # empty batch


def test_exponent_matches_frexp():
    for m in [np.float32(1.0), np.float32(0.75), np.float32(3.4e38), np.float32(1.5e-45), np.float32(1e-40), np.float32(1.17549435e-38),
              np.float32(6.0), np.float32(2.0 ** -130)]:
        bits = int(np.array([m], np.float32).view(np.uint32)[0])
        assert R.exponent_E(bits) == np.frexp(np.float64(m))[1], m
    assert R.det_K(1, 384, 512) == 22 and R.det_K(3, 20, 36) == 17 and R.det_K(1, 1, 1) == 4


def _check_bound(img_shape, flow, gout, k):
    got = R.resample_bwd_det(img_shape, flow, gout, k)
    exact, bound = R.exact_and_bound(img_shape, flow, gout, k)
    err = np.abs(got.astype(np.float64) - exact)
    finite = np.isfinite(exact)
    assert np.all(err[finite] <= bound[finite]), float(np.max(err[finite] / np.maximum(bound[finite], 1e-300)))
    return got, exact


def test_bound_negative_coordinates():
    """flows that send pixels to negative coordinates: truncation weights up to 4 (alpha = xf - (int)xf in (-1, 0])."""
    rng = np.random.default_rng(1)
    B, C, H, W = 2, 3, 12, 20
    flow = (rng.standard_normal((B, 2, H, W)) * 3 - 8).astype(np.float32)
    g = rng.standard_normal((B, C, H, W)).astype(np.float32)
    geom = R.scatter_geometry(flow[0], H, W, 1)
    assert max(float(np.max(np.abs(w))) for w, _ in geom[0]) > 2.0      # the weights really exceed 1
    _check_bound((B, C, H, W), flow, g, 1)


def test_bound_border_piles_k3():
    """every pixel pushed past the lower right border with k = 3: clamping piles up to 4 k^2 contributions of one pixel on one cell."""
    rng = np.random.default_rng(2)
    B, C, H, W = 1, 2, 9, 13
    flow = (rng.uniform(20, 30, (B, 2, H, W))).astype(np.float32)
    g = rng.standard_normal((B, C, H, W)).astype(np.float32)
    got, exact = _check_bound((B, C, 7, 11), flow, g, 3)
    assert np.count_nonzero(exact[0, 0]) == 1                          # everything landed on the corner cell


@pytest.mark.parametrize("scale", [2.0 ** -149, 1e-42, 3.0e38, 0.0])
def test_bound_extreme_magnitudes(scale):
    """a subnormal M, an M near FLT_MAX (contributions up to 4 M overflow fp32 only where the exact sum does), an all-zero plane."""
    rng = np.random.default_rng(3)
    B, C, H, W = 1, 2, 8, 16
    flow = (rng.standard_normal((B, 2, H, W)) * 2).astype(np.float32)
    g = (np.sign(rng.standard_normal((B, C, H, W))) * np.float32(scale)).astype(np.float32)
    if scale > 1e30:
        # M = 3e38 (E = 128, s < 0) on a few pixels, 1e36 elsewhere, small flows: every cell's sum stays below FLT_MAX
        flow = np.abs(flow) * 0.05
        g = (rng.standard_normal((B, C, H, W)) * 1e36).astype(np.float32)
        g[:, :, ::5, ::7] = np.float32(scale)
    got, exact = _check_bound((B, C, H, W), flow, g, 1)
    if scale == 0.0:
        assert not np.any(got) and not np.any(np.signbit(got))   # adds nothing: the zero prefill stays +0


def test_bound_channels_2_pow_pm40():
    rng = np.random.default_rng(4)
    B, C, H, W = 2, 3, 10, 14
    flow = (rng.standard_normal((B, 2, H, W)) * 2).astype(np.float32)
    g = rng.standard_normal((B, C, H, W)).astype(np.float32)
    g[:, 0] *= np.float32(2.0 ** 40)
    g[:, 2] *= np.float32(2.0 ** -40)
    _check_bound((B, C, H, W), flow, g, 1)


def test_nonfinite_plane_is_the_serial_oracle(oracle):
    rng = np.random.default_rng(5)
    B, C, H, W = 2, 3, 6, 9
    flow = (rng.standard_normal((B, 2, H, W)) * 2).astype(np.float32)
    g = rng.standard_normal((B, C, H, W)).astype(np.float32)
    g[1, 2, 3, 4] = np.inf
    g[0, 1, 0, 0] = np.nan
    img = np.zeros((B, C, H, W), np.float32)
    got = R.resample_bwd_det(img.shape, flow, g, 1)
    ref, _ = oracle.resample_bwd(img, flow, g)
    for b, c in [(1, 2), (0, 1)]:
        np.testing.assert_array_equal(got[b, c].view(np.uint32), ref[b, c].view(np.uint32))
    # the other planes are the fixed-point ones (a plane alone gives the same bits)
    alone = R.resample_bwd_det((1, 1, H, W), flow[:1], g[:1, :1], 1)
    np.testing.assert_array_equal(got[0, 0].view(np.uint32), alone[0, 0].view(np.uint32))


def test_mutation_sequential_fp32_differs(oracle):
    """At the GPU tests' converging-flow shapes the sequential fp32 sum (the oracle, the order a serial atomic path would take) differs
    from the fixed-point result in a large share of the cells: a bitwise GPU test against the helper cannot pass by accident with fp32
    atomics, whatever their order."""
    shares = {}
    for name, flow in [("sink", R.sink_flow(2, 96, 128, seed=3)), ("bench", R.bench_flow(2, 96, 128, seed=4))]:
        g = np.random.default_rng(6).standard_normal((2, 3, 96, 128)).astype(np.float32)
        img = np.zeros((2, 3, 96, 128), np.float32)
        det = R.resample_bwd_det(img.shape, flow, g, 1)
        seq, _ = oracle.resample_bwd(img, flow, g)
        touched = seq != 0
        shares[name] = float(np.mean(det[touched] != seq[touched]))
    print("share of cells where the sequential fp32 sum differs from the fixed-point one:", shares)
    assert shares["sink"] > 0.5 and shares["bench"] > 0.1, shares


def test_warp_diff_norm_cat_helper_against_float64():
    """the WarpDiffNormCat restatement: the concat slice plus a fixed-point scatter of g_warped, within the bound of the exact sum."""
    rng = np.random.default_rng(7)
    B, C, H, W = 2, 3, 10, 12
    pair = rng.standard_normal((B, 2 * C, H, W)).astype(np.float32)
    flow = (rng.standard_normal((B, 2, H, W)) * 2).astype(np.float32)
    outcat = rng.standard_normal((B, 3 * C + 3, H, W)).astype(np.float32)
    outcat[:, 3 * C + 2] = np.abs(outcat[:, 3 * C + 2]) + 0.5
    gcat = rng.standard_normal((B, 3 * C + 3, H, W)).astype(np.float32)
    got = R.warp_diff_norm_cat_grad_second(pair, flow, outcat, gcat)
    gw = R.warped_grad(pair, outcat, gcat)
    exact, bound = R.exact_and_bound((B, C, H, W), flow, gw, 1)
    exact = exact + gcat[:, C:2 * C].astype(np.float64)
    err = np.abs(got.astype(np.float64) - exact)
    assert np.all(err <= bound + np.abs(exact) * 2.0 ** -23)
