"""CPU-side checks of the smoothness library (include/flownet2_hip_smooth.h, libflownet2_hip_smooth.so; what it exports and
links is in tests/test_libraries_host.py): the seven headers in one translation unit, every rejection in front of a launch (host
pointers, no GPU), the refusals at the Python doors, the float64 reference against an independent PyTorch float64 composition
(values and flow gradient) and in closed form, the arithmetic header (csrc/smooth_arith.h) as a stand-alone program under the
undefined-behaviour sanitizer, and the kernels' scratch and LDS budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import fn2_capi
import smoothness_ref as RS

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
U = 2.0 ** -24


def test_seven_headers_in_one_translation_unit(tmp_path):
    """The smoothness header restates the codes unless one of the other six came first."""
    a, x, l, u, s, c, m = ("flownet2_hip.h", "flownet2_hip_ext.h", "flownet2_hip_lookup.h", "flownet2_hip_upsample.h", "flownet2_hip_splat.h",
                           "flownet2_hip_census.h", "flownet2_hip_smooth.h")
    for i, incs in enumerate(((a, x, l, u, s, c, m), (x, l, u, s, c, m), (a, l, u, s, c, m), (a, x, l, u, s, m), (a, x, l, u, c, m), (a, x, l, s, c, m), (l, u, s, c, m),
                              (u, s, c, m), (s, c, m), (c, m), (s, m), (u, m), (l, m), (x, m), (a, m), (m,), (m, m))):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in incs) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2M_TILE_H + FN2M_HALO_X + FN2M_MAX_ORDER + FN2M_MAX_FLOW_CHANNELS\n"
                       "          + FN2M_EDGE_GAUSSIAN + FN2M_BOUND_A + FN2M_BOUND_E];\n"
                       "char lds[FN2M_LDS_BYTES(5, 2, 0) == 24480 && FN2M_LDS_BYTES(7, 2, 1) == 40320 && FN2M_LDS_BYTES(9, 2, 1) == 51840 ? 1 : -1];\n"
                       "int (*fwd)(const void *, const void *, void *, int, int, int, int, int, int, int, float, float, void *) = fn2m_smoothness_forward;\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.smooth_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis1 = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    mis2 = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    shape = (1, 2, 3, 8, 16)   # N, F, C, H, W

    def fwd(ptrs, shp, order=1, edge=0, alpha=150.0, eps=0.001):
        return lib.fn2m_smoothness_forward(*ptrs, *shp, order, edge, alpha, eps, null)

    def bwd(ptrs, shp, order=1, edge=0, alpha=150.0, eps=0.001):
        return lib.fn2m_smoothness_backward(*ptrs, *shp, order, edge, alpha, eps, null)

    for call, n in ((fwd, 3), (bwd, 4)):
        good = [p] * n
        # 1. sizes, whatever else is wrong (NULL pointers, an order out of range)
        for shp in ((-1, 2, 3, 8, 16), (1, 0, 3, 8, 16), (1, 2, 0, 8, 16), (1, 2, -3, 8, 16), (1, 2, 3, 0, 16), (1, 2, 3, 8, 0), (1, 2, 3, -8, 16),
                    (0, 0, 3, 8, 16)):
            assert call([null] * n, shp, order=0) == EINVAL, shp
        # 2. a plane of 2^31 elements, 2^31 planes, 2^48 elements, 2^31 workgroups -- also with channel counts that are refused later
        for shp in ((1, 1, 1, 65536, 32768), (0, 1, 1, 65536, 32768), (65536, 32768, 1, 1, 1), (65536, 1, 32768, 1, 1),
                    (1 << 12, 1 << 12, 1, 1 << 12, 1 << 12), (1 << 24, 1, 1, 1, 1 << 15)):
            assert call([null] * n, shp, order=3) == EUNSUPPORTED, shp
        assert call([null] * n, (1, 1, 1, 32768, 65535)) == EINVAL      # just below 2^31: accepted, the NULL pointers are next
        # 3. an empty batch: nothing to do, whatever the pointers and the parameters
        assert call([null] * n, (0,) + shape[1:]) == OK
        assert call([mis1] * n, (0, 5, 2, 8, 16), order=7, edge=9, alpha=-1.0) == OK
        # 4. NULL pointers, also next to a misaligned one: NULL is reported first
        for i in range(n):
            ptrs = list(good)
            ptrs[i] = null
            ptrs[(i + 1) % n] = mis1
            assert call(ptrs, shape) == EINVAL, i
        # 5. alignment, in front of the parameters
        for i in range(n):
            for mis in (mis1, mis2):
                ptrs = list(good)
                ptrs[i] = mis
                assert call(ptrs, shape, order=0) == EALIGN, i
        # 6. the parameters last of all
        for C in (2, 4, 64):
            assert call(good, (1, 2, C, 8, 16)) == EINVAL, C
        for F in (5, 6, 64):
            assert call(good, (1, F, 3, 8, 16)) == EINVAL, F
        for order in (0, 3, -1, 100):
            assert call(good, shape, order=order) == EINVAL, order
            assert call(good[:-1] + [mis2], shape, order=order) == EALIGN
            assert call(good, (0,) + shape[1:], order=order) == OK
        for edge in (-1, 2, 7):
            assert call(good, shape, edge=edge) == EINVAL, edge
        for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-30):
            assert call(good, shape, alpha=bad) == EINVAL, bad
            assert call(good, shape, eps=bad) == EINVAL, bad
    with pytest.raises(RuntimeError):
        fn2_capi.check(EUNSUPPORTED, "fn2m_smoothness_forward")


def test_cpu_tensors_and_bad_arguments_are_refused():
    import smoothness_cuda
    from networks.smoothness_package import EdgeAwareSmoothness, SmoothnessFunction, SmoothnessLoss, smoothness_map
    f, im = torch.zeros(2, 2, 8, 9), torch.zeros(2, 3, 8, 9)
    e = torch.zeros(0)
    go = torch.zeros(2, 2, 8, 9)
    doors = (lambda a, b, k=1: smoothness_cuda.forward(a, b, e, k),
             lambda a, b, k=1: smoothness_cuda.backward(a, b, go, e, k),
             lambda a, b, k=1: smoothness_cuda.forward_alloc(a, b, k),
             lambda a, b, k=1: smoothness_cuda.backward_alloc(a, b, go, k),
             lambda a, b, k=1: smoothness_cuda.apply(a, b, k),
             lambda a, b, k=1: SmoothnessFunction.apply(a, b, k),
             lambda a, b, k=1: smoothness_map(a, b, k),
             lambda a, b, k=1: smoothness_map(a, b, order=k, edge_weighting="gaussian", alpha=10.0, eps=0.0),
             lambda a, b, k=1: EdgeAwareSmoothness(k)(a, b),
             lambda a, b, k=1: SmoothnessLoss(k)(a, b))
    for door in doors:
        for k in (1, 2):
            with pytest.raises(RuntimeError, match="no CPU implementation"):
                door(f, im, k)
        # bad arguments are reported as such on any device, at every door
        for shp in ((1, 3, 8, 9), (2, 3, 9, 9), (2, 3, 8, 8)):
            with pytest.raises(RuntimeError, match="must have the batch, height and width of flow"):
                door(f, torch.zeros(shp))
        for C in (2, 4):
            with pytest.raises(RuntimeError, match="channels, expected 1 \\(grey\\)"):
                door(f, torch.zeros(2, C, 8, 9))
        for F in (5, 8):
            with pytest.raises(RuntimeError, match="channels, expected 1 to 4"):
                door(torch.zeros(2, F, 8, 9), im)
        with pytest.raises(RuntimeError, match="4-D"):
            door(f[0], im[0])
        for dt, name in ((torch.float16, "Half"), (torch.bfloat16, "BFloat16"), (torch.float64, "Double")):
            with pytest.raises(RuntimeError, match=rf"flow must be float32, got {name}.*\.float\(\)"):
                door(f.to(dt), im)
            with pytest.raises(RuntimeError, match=rf"image must be float32, got {name}.*\.float\(\)"):
                door(f, im.to(dt))
        # the image gets no gradient: asking for one is an error, not a silent None
        with pytest.raises(RuntimeError, match="image requires a gradient"):
            door(f, im.clone().requires_grad_(True))
    # the parameters: RuntimeError at the extension's doors, ValueError at the package's
    for order in (0, 3, -1):
        with pytest.raises(RuntimeError, match=f"order {order} is not 1 or 2"):
            smoothness_cuda.forward_alloc(f, im, order)
        for make in (lambda: smoothness_map(f, im, order), lambda: EdgeAwareSmoothness(order), lambda: SmoothnessLoss(order),
                     lambda: SmoothnessFunction.apply(f, im, order)):
            with pytest.raises(ValueError, match="is not 1 or 2"):
                make()
    for edge in (2, -1):
        with pytest.raises(RuntimeError, match="edge_weighting .* is not 0"):
            smoothness_cuda.forward_alloc(f, im, 1, edge)
    for edge in ("charbonnier", 0, None):
        for make in (lambda: smoothness_map(f, im, 1, edge), lambda: EdgeAwareSmoothness(1, edge), lambda: SmoothnessLoss(2, edge)):
            with pytest.raises(ValueError, match="is not 'exponential' or 'gaussian'"):
                make()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="alpha .* is not a finite float >= 0"):
            smoothness_cuda.forward_alloc(f, im, 1, 0, bad)
        with pytest.raises(RuntimeError, match="eps .* is not a finite float >= 0"):
            smoothness_cuda.apply(f, im, 1, 0, 150.0, bad)
        for make in (lambda: smoothness_map(f, im, alpha=bad), lambda: EdgeAwareSmoothness(alpha=bad), lambda: SmoothnessLoss(alpha=bad)):
            with pytest.raises(ValueError, match="alpha .* is not a finite number >= 0"):
                make()
        for make in (lambda: smoothness_map(f, im, eps=bad), lambda: EdgeAwareSmoothness(eps=bad), lambda: SmoothnessLoss(eps=bad)):
            with pytest.raises(ValueError, match="eps .* is not a finite number >= 0"):
                make()
    m = RS.header_macros()
    assert (smoothness_cuda.MAX_ORDER, smoothness_cuda.MAX_FLOW_CHANNELS) == (2, 4) == (m["FN2M_MAX_ORDER"], m["FN2M_MAX_FLOW_CHANNELS"])
    assert (smoothness_cuda.EDGE_EXPONENTIAL, smoothness_cuda.EDGE_GAUSSIAN) == (0, 1) == (m["FN2M_EDGE_EXPONENTIAL"], m["FN2M_EDGE_GAUSSIAN"])
    assert fn2_capi.FN2M_EDGE == {"exponential": 0, "gaussian": 1}


def _independent(flow, image, k, edge, alpha, eps):
    """An independent float64 composition: UFlow's image_grads with stride k and its flow gradients applied k times, written with
    slices per direction -- shares no code with smoothness_ref."""
    N, F, H, W = flow.shape
    out = torch.zeros(N, 2, H, W, dtype=flow.dtype)
    if W > k:
        gx = alpha * (image[..., k:] - image[..., :-k])
        wx = torch.exp(-torch.mean(torch.abs(gx) if edge == "exponential" else gx ** 2, 1))
        d = flow[..., 1:] - flow[..., :-1]
        if k == 2:
            d = d[..., 1:] - d[..., :-1]
        out[:, 0, :, :W - k] = wx * torch.sqrt(d ** 2 + eps ** 2).sum(1)
    if H > k:
        gy = alpha * (image[:, :, k:] - image[:, :, :-k])
        wy = torch.exp(-torch.mean(torch.abs(gy) if edge == "exponential" else gy ** 2, 1))
        d = flow[:, :, 1:] - flow[:, :, :-1]
        if k == 2:
            d = d[:, :, 1:] - d[:, :, :-1]
        out[:, 1, :H - k] = wy * torch.sqrt(d ** 2 + eps ** 2).sum(1)
    return out


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("edge", RS.EDGES)
@pytest.mark.parametrize("order", [1, 2])
def test_reference_is_the_pytorch_composition(C, edge, order):
    """Values and the flow gradient of the float64 reference against autograd of an independent float64 composition, to 1e-12
    relative; the file's own ``compose`` in float64 agrees too, and in fp32 it stays below a third of both bounds."""
    for family, eps, F in ((0, 0.001, 2), (1, 0.01, 3)):
        shape = (2, F, C, 11, 13)
        flow, image, go, alpha = RS.inputs(shape, family, 100 + 10 * order + C)
        out, fb = RS.forward(flow, image, order, edge, alpha, eps)
        grad, gb = RS.backward(flow, image, go, order, edge, alpha, eps)
        a32, e32 = float(np.float32(alpha)), float(np.float32(eps))
        for fn in (lambda f, i: _independent(f, i, order, edge, a32, e32), lambda f, i: RS.compose(f, i, order, edge, alpha, eps)):
            t = torch.from_numpy(flow.astype(np.float64)).requires_grad_(True)
            got = fn(t, torch.from_numpy(image.astype(np.float64)))
            got.backward(torch.from_numpy(go.astype(np.float64)))
            assert np.abs(got.detach().numpy() - out).max() <= 1e-12 * np.abs(out).max()
            assert np.abs(t.grad.numpy() - grad).max() <= 1e-12 * np.abs(grad).max()
        assert out.max() > 0 and np.abs(grad).max() > 0 and (fb[out > 0] > 0).all() and (gb[grad != 0] > 0).all()
        # the composition in fp32: the family's own error against the bounds
        t = torch.from_numpy(flow).requires_grad_(True)
        o32 = RS.compose(t, torch.from_numpy(image), order, edge, alpha, eps)
        o32.backward(torch.from_numpy(go))
        ef, eg = np.abs(o32.detach().numpy().astype(np.float64) - out), np.abs(t.grad.numpy().astype(np.float64) - grad)
        assert (ef <= fb / 3).all() and (eg <= gb / 3).all(), (float((ef / np.where(fb > 0, fb, 1)).max()), float((eg / np.where(gb > 0, gb, 1)).max()))
        assert (ef[fb == 0] == 0).all() and (eg[gb == 0] == 0).all()


def test_reference_closed_forms():
    rng = np.random.default_rng(5)
    for (C, F), order, edge in (((1, 1), 1, "exponential"), ((3, 2), 2, "gaussian"), ((3, 4), 1, "gaussian"), ((1, 3), 2, "exponential")):
        shape = (2, F, C, 12, 15)
        flow, image, go, alpha = RS.inputs(shape, 0, 7 + order)
        N, _, _, H, W = shape
        k, eps = order, float(np.float32(0.001))
        # a constant flow: out = w F eps on the valid cells, and an exactly zero gradient
        const = np.full_like(flow, 3.25)
        out, _ = RS.forward(const, image, order, edge, alpha, 0.001)
        grad, gb = RS.backward(const, image, go, order, edge, alpha, 0.001)
        q = RS._direction(const, image, 3, order, edge, alpha, 0.001)
        assert np.abs(out[:, 0:1, :, :W - k] - q["w"] * F * eps).max() <= 1e-18 and (grad == 0).all() and gb.max() > 0
        assert (out[:, 0, :, W - k:] == 0).all() and (out[:, 1, H - k:] == 0).all() and (out[:, 0, :, :W - k] > 0).all()
        # a constant image: w = 1 exactly, out = sum_f rho
        flat = np.full_like(image, 0.375)
        out, _ = RS.forward(flow, flat, order, edge, alpha, 0.001)
        qx = RS._direction(flow, flat, 3, order, edge, alpha, 0.001)
        assert (qx["w"] == 1.0).all() and np.array_equal(out[:, 0:1, :, :W - k], qx["rho"].sum(1, keepdims=True))
        # grad_out on the cells that carry no term reaches nothing, NaN included
        go_nan = go.copy()
        go_nan[:, 0, :, W - k:] = np.nan
        go_nan[:, 1, H - k:] = np.nan
        g1, b1 = RS.backward(flow, image, go, order, edge, alpha, 0.001)
        g2, b2 = RS.backward(flow, image, go_nan, order, edge, alpha, 0.001)
        assert np.array_equal(g1, g2) and np.array_equal(b1, b2) and np.abs(g1).max() > 0
    # order 2 on an affine flow with dyadic slopes: d = 0 exactly, so out = w F eps and, with eps = 0, everything is 0
    yy, xx = np.mgrid[0:9, 0:14].astype(np.float32)
    affine = np.stack([0.5 * xx - 0.25 * yy + 3.0, -1.75 * xx + 2.0 * yy])[None]
    image = (0.5 + 0.05 * (rng.random((1, 3, 9, 14)) - 0.5)).astype(np.float32)
    go = rng.standard_normal((1, 2, 9, 14)).astype(np.float32)
    for axis in (2, 3):
        assert (RS._direction(affine, image, axis, 2, "exponential", 150.0, 0.0)["d"] == 0).all()
    out, fb = RS.forward(affine, image, 2, "exponential", 150.0, 0.0)
    grad, gb = RS.backward(affine, image, go, 2, "exponential", 150.0, 0.0)
    assert (out == 0).all() and (grad == 0).all() and (gb[:, :, 2:-2, 2:-2] > 0).all()
    assert (fb[:, 0, :, :12] > 0).all() and (fb[:, 0, :, 12:] == 0).all()      # the S term: the second difference cancelled
    out, _ = RS.forward(affine, image, 2, "exponential", 150.0, 0.001)
    qx = RS._direction(affine, image, 3, 2, "exponential", 150.0, 0.001)
    assert np.abs(out[:, 0:1, :, :12] - qx["w"] * 2 * float(np.float32(0.001))).max() <= 1e-18
    # order 1 on the same flow: d is the slope, rho' its sign with eps = 0
    q1 = RS._direction(affine, image, 3, 1, "exponential", 150.0, 0.0)
    assert (q1["d"][0, 0] == 0.5).all() and (q1["d"][0, 1] == -1.75).all() and (q1["drho"][0, 0] == 1).all() and (q1["drho"][0, 1] == -1).all()
    # planes too small for the stencil: all zero, also in the composition
    for shape, order in (((1, 1, 1, 1, 1), 1), ((1, 2, 3, 2, 2), 2), ((1, 2, 3, 1, 6), 1), ((1, 2, 1, 5, 2), 2)):
        flow, image, go, alpha = RS.inputs(shape, 0, 3)
        out, fb = RS.forward(flow, image, order)
        grad, gb = RS.backward(flow, image, go, order)
        H, W = shape[3:]
        if W <= order:
            assert (out[:, 0] == 0).all() and (fb[:, 0] == 0).all()
        if H <= order:
            assert (out[:, 1] == 0).all() and (fb[:, 1] == 0).all()
        if W <= order and H <= order:
            assert (grad == 0).all() and (gb == 0).all()
        t = RS.compose(torch.from_numpy(flow), torch.from_numpy(image), order)
        assert t.shape == out.shape and np.abs(t.numpy() - out).max() <= 1e-5 * max(1.0, out.max())
    # SmoothnessLoss's reduction is UFlow's two means
    for shape, order in (((2, 2, 3, 7, 9), 1), ((1, 4, 1, 6, 5), 2), ((1, 2, 3, 2, 6), 2), ((1, 1, 1, 1, 1), 1)):
        flow, image, go, alpha = RS.inputs(shape, 1, 11)
        out, _ = RS.forward(flow, image, order, "gaussian", alpha, 0.01)
        want = RS.compose_loss(torch.from_numpy(flow.astype(np.float64)), torch.from_numpy(image.astype(np.float64)), order, "gaussian", alpha, 0.01)
        assert abs(RS.loss_of(out, shape[1], order) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


_ARITH_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "smooth_arith.h"
static float arg(unsigned bits) { float v; std::memcpy(&v, &bits, 4); return v; }
int main()
{
    char kind;
    unsigned a, b, c, d;
    while (std::scanf(" %c %x %x %x %x", &kind, &a, &b, &c, &d) == 5) {
        if (kind == 'e') {   // dI, alpha: the two edge terms of one channel and their weights
            const float x = smooth_edge_term(arg(a), arg(b), 0), g = smooth_edge_term(arg(a), arg(b), 1);
            std::printf("%a %a %a %a\n", x, g, smooth_weight(x), smooth_weight(g));
        } else if (kind == 'm') {   // three terms: their mean and its weight
            const float e = smooth_mean3(arg(a), arg(b), arg(c));
            std::printf("%a %a\n", e, smooth_weight(e));
        } else {   // f0, f1, f2, eps2: both differences, rho and rho' of each
            const float d1 = smooth_d1(arg(a), arg(b)), d2 = smooth_d2(arg(a), arg(b), arg(c));
            std::printf("%a %a %a %a %a %a\n", d1, d2, smooth_rho(d1, arg(d)), smooth_drho(d1, arg(d)), smooth_rho(d2, arg(d)), smooth_drho(d2, arg(d)));
        }
    }
    return 0;
}
"""


def test_arithmetic_header_under_the_undefined_behaviour_sanitizer(tmp_path):
    """csrc/smooth_arith.h in a stand-alone program (its own main), built with the undefined-behaviour sanitizer without recovery
    and without contraction, on edge values: the edge terms and differences bit for bit against the numpy float32 restatement, the
    weight, rho and rho' within their shares of the header's derivation against float64."""
    src, exe = tmp_path / "arith.cpp", tmp_path / "arith"
    src.write_text(_ARITH_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                        "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    f32 = np.float32
    bits = lambda v: int(np.asarray(v, f32).view(np.uint32))     # noqa: E731
    same = lambda got, want: f32(got).view(np.uint32) == f32(want).view(np.uint32)     # noqa: E731
    rng = np.random.default_rng(9)
    dIs = [f32(v) for v in (0.0, -0.0, 1e-30, -1e-40, 0.05, -0.05, 0.37, -0.75, 1.0, 3.0)] + list((rng.random(20).astype(f32) - f32(0.5)))
    alphas = [f32(v) for v in (0.0, 1.0, 10.0, 150.0)]
    fs = [f32(v) for v in (0.0, -0.0, 1e-30, -1e-40, 0.125, -64.0, 3.3, 2.0 ** 59, -2.0 ** 59, 17.77, 17.78)]
    eps2s = [f32(0.0), f32(f32(0.001) * f32(0.001)), f32(f32(0.01) * f32(0.01)), f32(1.0)]
    lines, cases = [], []
    for dI in dIs:
        for al in alphas:
            lines.append("e %08x %08x 0 0" % (bits(dI), bits(al)))
            cases.append(("e", dI, al))
    for _ in range(40):
        t = (rng.random(3) * rng.choice([0.0, 1e-3, 1.0, 50.0], 3)).astype(f32)
        lines.append("m %08x %08x %08x 0" % tuple(bits(v) for v in t))
        cases.append(("m",) + tuple(t))
    trip = [(a, b, c) for a in fs for b in fs[:8] for c in fs[2:7]] + [tuple((20 * rng.standard_normal(3)).astype(f32)) for _ in range(60)]
    for i, (a, b, c) in enumerate(trip):
        e2 = eps2s[i % 4]
        lines.append("d %08x %08x %08x %08x" % (bits(a), bits(b), bits(c), bits(e2)))
        cases.append(("d", a, b, c, e2))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(cases)

    def weight_ok(w, e32):
        """exp2 of the scaled argument: 1.25 e u from the scaling, 2 u from exp2 (libm here), the flush floor."""
        e = float(e32)
        want = np.exp(-e)
        return abs(w - want) <= U * (2 + 1.25 * e) * want + 2.0 ** -126 and 0.0 <= w <= 1.0

    for case, line in zip(cases, out):
        got = [float.fromhex(t) for t in line.split()]
        if case[0] == "e":
            _, dI, al = case
            t = f32(al * dI)
            assert same(got[0], np.abs(t)) and same(got[1], f32(t * t)), case
            assert weight_ok(got[2], got[0]) and weight_ok(got[3], got[1]), case
            if float(t) == 0.0:
                assert got[2] == 1.0 and got[3] == 1.0, "exp(-0) must be exactly 1"
        elif case[0] == "m":
            _, a, b, c = case
            assert same(got[0], f32(f32(f32(a + b) + c) * f32(1.0 / 3.0))), case
            assert abs(got[0] - (float(a) + float(b) + float(c)) / 3) <= 4 * U * got[0] + 2.0 ** -149 and weight_ok(got[1], got[0]), case
        else:
            _, a, b, c, e2 = case
            d1, d2 = f32(b - a), f32(f32(c - b) - f32(b - a))
            assert same(got[0], d1) and same(got[1], d2), case
            for d, rho, drho in ((d1, got[2], got[3]), (d2, got[4], got[5])):
                d64, e64 = float(d), float(e2)
                want = np.sqrt(d64 * d64 + e64)
                if e64 == 0.0:
                    assert rho == abs(d64) and drho == np.sign(d64), case      # the L1 form, exactly
                    continue
                assert abs(rho - want) <= 3 * U * want + 2.0 ** -149, case                         # d d, the sum (halved by the root), the root
                assert abs(drho - d64 / want) <= 4 * U * abs(d64 / want) + 2.0 ** -149 and abs(drho) <= 1.0 + 4 * U, case
                if d64 == 0.0:
                    assert drho == 0.0 and same(rho, np.sqrt(e2)), case


def test_kernels_use_no_scratch_and_their_lds_is_the_headers_formula(tmp_path):
    """0 bytes of scratch for every instantiation -- order 1, 2 x C 1, 3 x F 1 .. 4, forward and backward: 32 kernels -- and each
    kernel's LDS is exactly FN2M_LDS_BYTES: F + C planes (forward) or F + C + 2 (backward); device code only, the library's own
    flags."""
    import build
    src = os.path.join(PKG, "csrc", "smooth.hip")
    r = subprocess.run([build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "smooth.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S*smooth_\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", r.stderr, flags=re.S)
    names = [k for k, _, _ in kernels]
    assert sum("smooth_fwd" in k for k in names) == 16 and sum("smooth_bwd" in k for k in names) == 16 and len(names) == 32, names
    m = RS.header_macros()
    assert (m["FN2M_TILE_H"], m["FN2M_TILE_W"], m["FN2M_HALO_X"]) == (16, 64, 4)
    seen = set()
    for name, body, lds in kernels:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
        assert scratch == 0, f"{name} spills {scratch} bytes per lane"
        kind, k, C, F = re.search(r"smooth_(fwd|bwd)ILi(\d)ELi(\d)ELi(\d)E", name).groups()
        k, C, F = int(k), int(C), int(F)
        bwd = kind == "bwd"
        planes = F + C + (2 if bwd else 0)
        want = planes * 4 * (16 + (2 * k if bwd else k)) * (64 + (8 if bwd else 4))
        assert want == RS.lds_bytes(planes, k, bwd) and int(lds) == want, f"{name} uses {lds} bytes of LDS, expected {want}"
        seen.add((kind, k, C, F))
    assert seen == {(d, k, C, F) for d in ("fwd", "bwd") for k in (1, 2) for C in (1, 3) for F in (1, 2, 3, 4)}
    assert RS.lds_bytes(5, 2, False) == 24480 and RS.lds_bytes(9, 2, True) == 51840 <= 64 * 1024


# ------------------------------------------------------------------ the input families and the corrected gradient bound
_FAMILY_SHAPES = ((1, 1, 1, 17, 65), (2, 2, 3, 33, 130))


def _family_eps(family):
    return RS.GRADED_EPS if family == "graded" else (0.0, 0.001)


def _worst(err, bound):
    """Largest err / bound where the bound is positive; where it is 0 the error must be 0."""
    assert (err[bound == 0] == 0).all()
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def _emulated_ratios(shape, family, order, edge, eps, mutate=None):
    """(forward, gradient against the first-order bound, gradient against the corrected bound, corrected / first-order) of the
    float32 emulation of the header's operation list."""
    flow, image, go, alpha = RS.inputs(shape, family, 77 + shape[3])
    out, fb = RS.forward(flow, image, order, edge, alpha, eps)
    grad, gb, gc = RS.backward(flow, image, go, order, edge, alpha, eps, corrected=True)
    assert np.isfinite(fb).all() and np.isfinite(gc).all() and (gc >= gb).all(), "(a): the corrected bound is below the first-order one"
    o, g = RS.emulate(flow, image, go, order, edge, alpha, eps, mutate)
    eg = np.abs(g.astype(np.float64) - grad)
    old = float((eg / np.where(gb > 0, gb, 2.0 ** -1074)).max())
    grow = float((gc[gb > 0] / gb[gb > 0]).max()) if (gb > 0).any() else 1.0
    return _worst(np.abs(o.astype(np.float64) - out), fb), old, _worst(eg, gc), grow


def test_input_families_keep_their_conditions():
    """Every named family asserts in ``inputs`` what it is for; here at every shape the GPU tests use, and a family made benign
    is refused."""
    for shape in _FAMILY_SHAPES + ((2, 3, 3, 20, 132),):
        for family in RS.NEW_FAMILIES:
            flow, image, go, alpha = RS.inputs(shape, family, 3)
            assert flow.dtype == image.dtype == go.dtype == np.float32 and flow.shape == shape[:2] + shape[3:]
    flow, image, go, alpha = RS.inputs(_FAMILY_SHAPES[1], "ramp", 3)
    plain = RS.inputs(_FAMILY_SHAPES[1], 0, 3)[0]
    for family, bad in (("ramp", plain), ("offset", plain), ("graded", plain)):
        with pytest.raises(AssertionError):
            RS.check_family(family, bad, image, alpha)
    with pytest.raises(AssertionError):
        RS.check_family("edges", flow, np.full_like(image, 0.5), alpha)
    with pytest.raises(AssertionError):
        RS.check_family("alpha0", flow, image, 150.0)


def test_emulation_stays_inside_the_corrected_bound_and_leaves_the_first_order_one_on_ramp():
    """(a) the corrected gradient bound is nowhere below the first-order one of ABI 1; (b) on the two original families it
    exceeds it by at most 1.1 (printed); (c) the float32 emulation of the header's list stays inside the forward
    bound and the corrected gradient bound on every family and every (order, edge, eps); (d) on ``ramp`` with order 2 it
    exceeds the first-order bound -- by 10^5 at eps = 0 -- which is why the header changed."""
    grow_old, left = 1.0, {}
    for family in (0, 1) + RS.NEW_FAMILIES:
        worst = [0.0, 0.0, 0.0]
        for shape in _FAMILY_SHAPES:
            for order in (1, 2):
                for edge in RS.EDGES:
                    for eps in ((0.001, 0.01) if family in (0, 1) else _family_eps(family)):
                        f, old, new, grow = _emulated_ratios(shape, family, order, edge, eps)
                        worst = [max(a, b) for a, b in zip(worst, (f, old, new))]
                        if family in (0, 1):
                            grow_old = max(grow_old, grow)
                        if family == "ramp" and order == 2:
                            left[eps] = max(left.get(eps, 0.0), old)
        print(f"emulation, family {family}: forward {worst[0]:.3f}, gradient / first-order bound {worst[1]:.3g}, / corrected bound {worst[2]:.3f}")
        assert worst[0] <= 1 and worst[2] <= 1, (family, worst)
        if family in (0, 1):
            assert worst[1] <= 0.5
    print(f"corrected / first-order gradient bound on the original families: at most {grow_old:.3f}")
    assert 1.0 <= grow_old <= 1.1
    print("ramp, order 2: emulation / first-order bound", {k: f"{v:.3g}" for k, v in left.items()})
    assert left[0.0] > 1e4 and left[0.001] > 10


@pytest.mark.parametrize("mutate,family,order,eps", [("d2_regrouped", "offset", 2, 0.001), ("clamped_exponent", "edges", 1, 0.001)])
def test_a_planted_mistake_passes_the_original_families_and_fails_a_new_one(mutate, family, order, eps):
    """Teeth, on the forward: the second difference regrouped as (f[x + 2] - 2 f[x + 1]) + f[x] and exp2's argument clamped
    at -125 (no weight is flushed) stay inside half of the forward bound on both original families -- and leave it on ``offset`` and on
    ``edges``, where the unchanged emulation stays inside."""
    shape = _FAMILY_SHAPES[1]
    for old in (0, 1):
        for edge in RS.EDGES:
            f = _emulated_ratios(shape, old, order, edge, eps, mutate)[0]
            assert f <= 0.5, (old, edge, f)
    f = _emulated_ratios(shape, family, order, "exponential", eps, mutate)[0]
    clean = _emulated_ratios(shape, family, order, "exponential", eps)[0]
    print(f"{mutate} on {family}: forward error / bound {f:.3g}, without the mistake {clean:.3f}")
    assert f > 1 and clean <= 1
