"""CPU-side checks of ConvexUpsample's library (include/flownet2_hip_upsample.h, libflownet2_hip_upsample.so; what it exports
and links is in tests/test_libraries_host.py): its workspace size, the four headers in one translation unit, every rejection in front of a launch
(host pointers, no GPU), the refusals at the Python doors, the float64 reference against RAFT's composition (values and both
gradients) and in closed form, and the kernels' scratch and LDS budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import convex_upsample_ref as RU
import fn2_capi

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
GEOMETRIES = [(1, 1, 1), (3, 5, 2), (4, 7, 3)]   # H, W, C
FACTORS = [2, 4, 8]


def test_workspace_bytes():
    ws = fn2_capi.upsample_lib().fn2u_convex_upsample_backward_workspace_bytes
    assert ws(8, 2, 55, 128) == 9 * 4 * 8 * 2 * 55 * 128
    assert ws(0, 2, 55, 128) == 0 and ws(1, 1, 1, 1) == 36
    for bad in ((-1, 2, 4, 4), (1, 0, 4, 4), (1, 5, 4, 4), (1, 2, 0, 4), (1, 2, 4, 0), (1, 2, 65536, 32768)):
        assert ws(*bad) == 0, bad


def test_four_headers_in_one_translation_unit(tmp_path):
    """The upsample header restates the codes unless one of the other three came first."""
    a, x, l, u = "flownet2_hip.h", "flownet2_hip_ext.h", "flownet2_hip_lookup.h", "flownet2_hip_upsample.h"
    for i, incs in enumerate(((a, x, l, u), (x, l, u), (a, l, u), (a, x, u), (l, u), (x, u), (a, u), (u,), (u, u))):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in incs) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2U_MAX_CHANNELS + FN2U_GROUPS(8) + FN2U_K0_F];\n"
                       "size_t (*ws)(int, int, int, int) = fn2u_convex_upsample_backward_workspace_bytes;\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.upsample_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis2 = ctypes.c_void_p(ctypes.addressof(buf) + 2)    # aligned for a 16-bit element, not for float
    mis1 = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    sc = ctypes.c_float(8.0)
    shape = (1, 2, 8, 16)   # B, C, H, W

    def f(ptrs, dt, shp, fac):
        return lib.fn2u_convex_upsample_forward(*ptrs, dt, *shp, fac, sc, null)

    def b(ptrs, dt, shp, fac):
        return lib.fn2u_convex_upsample_backward(*ptrs, dt, *shp, fac, sc, null)

    # (call, tensor pointers, index of mask-typed pointers, has a workspace)
    for call, n, masky, has_ws in ((f, 3, (1,), False), (b, 5, (1, 4), True)):
        nn = n + has_ws
        good = [p] * nn
        # 1. the mask's dtype first of all, whatever else is wrong
        for dt in (2, 7, -1, 4):
            assert call([null] * nn, dt, (1, 0, 8, 16), 3) == EDTYPE, dt
        for dt in (0, 1, 3):
            # 2. the factor, before the sizes
            for fac in (0, 1, 3, 5, 6, 7, 16, -2):
                assert call([null] * nn, dt, (1, 0, 8, 16), fac) == EINVAL, fac
            # 3. sizes
            for shp in ((-1, 2, 8, 16), (1, 0, 8, 16), (1, -2, 8, 16), (1, 2, 0, 16), (1, 2, 8, 0), (1, 2, -8, 16), (1, 9, 0, 16)):
                assert call([null] * nn, dt, shp, 8) == EINVAL, shp
            # 4. more channels than the kernels hold, an output plane beyond 31 bits
            assert call([null] * nn, dt, (1, 5, 8, 16), 8) == EUNSUPPORTED
            assert call([null] * nn, dt, (1, 1, 65536, 32768), 2) == EUNSUPPORTED
            assert call([null] * nn, dt, (1, 1, 8192, 4096), 8) == EUNSUPPORTED      # 2^31 exactly
            assert call([null] * nn, dt, (1, 1, 8192, 4096), 4) == EINVAL            # 2^29: accepted, the NULL pointers are next
            # 5. an empty batch: nothing to do, whatever the pointers
            assert call([null] * nn, dt, (0,) + shape[1:], 8) == OK
            assert call([mis1] * nn, dt, (0,) + shape[1:], 8) == OK
            # 6. NULL tensor pointers, also next to a misaligned one: NULL is reported first
            for i in range(n):
                ptrs = list(good)
                ptrs[i] = null
                ptrs[(i + 1) % n] = mis1
                assert call(ptrs, dt, shape, 8) == EINVAL, i
            # 7. alignment to the element size
            for i in range(nn):
                ptrs = list(good)
                ptrs[i] = mis1
                assert call(ptrs, dt, shape, 8) == EALIGN, i
                if dt == 0 or i not in masky:
                    ptrs[i] = mis2
                    assert call(ptrs, dt, shape, 8) == EALIGN, (dt, i)
            # 8. the workspace: NULL is reported after every alignment; 2 bytes are enough for a 16-bit mask and its gradient
            if has_ws:
                ptrs = list(good)
                ptrs[n] = null
                assert call(ptrs, dt, shape, 8) == EINVAL
                if dt != 0:
                    for i in masky:
                        ptrs[i] = mis2
                    assert call(ptrs, dt, shape, 8) == EINVAL
                ptrs[0] = mis1
                assert call(ptrs, dt, shape, 8) == EALIGN
    with pytest.raises(RuntimeError):
        fn2_capi.check(EUNSUPPORTED, "fn2u_convex_upsample_forward")


def test_cpu_tensors_and_bad_arguments_are_refused():
    import convex_upsample_cuda
    from networks.upsample_package import ConvexUpsample, ConvexUpsampleFunction, upsample_flow
    fl, mk = torch.zeros(2, 2, 3, 5), torch.zeros(2, 9 * 64, 3, 5)
    e = torch.zeros(0)
    go = torch.zeros(2, 2, 24, 40)
    doors = (lambda a, m, f=8: convex_upsample_cuda.forward(a, m, e, f, 8.0),
             lambda a, m, f=8: convex_upsample_cuda.backward(a, m, go, e, e.clone(), f, 8.0),
             lambda a, m, f=8: convex_upsample_cuda.forward_alloc(a, m, f, 8.0),
             lambda a, m, f=8: convex_upsample_cuda.backward_alloc(a, m, go, f, 8.0),
             lambda a, m, f=8: convex_upsample_cuda.apply(a, m, f, 8.0),
             lambda a, m, f=8: ConvexUpsampleFunction.apply(a, m, f, 8.0),
             lambda a, m, f=8: ConvexUpsample(f)(a, m))
    for door in doors:
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            door(fl, mk)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        upsample_flow(fl, mk)
    # bad arguments are reported as such on any device, at every door
    for door in doors:
        for bad_f in (1, 3, 16, 0, -8):
            with pytest.raises(RuntimeError, match="is not 2, 4 or 8"):
                door(fl, mk, bad_f)
        for ch in (9 * 64 + 1, 9 * 16, 64, 9):
            with pytest.raises(RuntimeError, match="expected 9 \\* factor\\^2 = 576"):
                door(fl, torch.zeros(2, ch, 3, 5))
        with pytest.raises(RuntimeError, match="expected 9 \\* factor\\^2 = 144"):
            door(fl, mk, 4)
        for shp in ((1, 576, 3, 5), (2, 576, 4, 5), (2, 576, 3, 6)):
            with pytest.raises(RuntimeError, match="must have the batch size, height and width"):
                door(fl, torch.zeros(shp))
        with pytest.raises(RuntimeError, match="4-D"):
            door(fl[0], mk)
        with pytest.raises(RuntimeError, match="channels, 1 .. 4 are supported"):
            door(torch.zeros(2, 5, 3, 5), mk)
        with pytest.raises(RuntimeError, match="flow must be float32"):
            door(fl.half(), mk)
        with pytest.raises(RuntimeError, match="mask must be float32, float16 or bfloat16"):
            door(fl, mk.double())
    for ch in (9 * 64 + 1, 9, 9 * 9, 9 * 256, 8 * 64):
        with pytest.raises(ValueError, match="9 f\\^2"):
            upsample_flow(fl, torch.zeros(2, ch, 3, 5))
    with pytest.raises(ValueError, match="9 f\\^2"):
        upsample_flow(fl, torch.zeros(9 * 64, 3, 5))
    with pytest.raises(RuntimeError, match="must have the batch size, height and width"):
        upsample_flow(fl, torch.zeros(2, 9 * 16, 3, 6))
    m = ConvexUpsample()
    assert (m.factor, m.scale) == (8, None) and "factor=8" in repr(m) and "scale=None" in repr(m)
    m = ConvexUpsample(4, 2.5)
    assert (m.factor, m.scale) == (4, 2.5) and "factor=4, scale=2.5" in repr(m)


def _case(geo, f, seed):
    H, W, C = geo
    rng = np.random.default_rng(seed)
    flow = (10 * rng.standard_normal((2, C, H, W))).astype(np.float32)
    mask = (3 * rng.standard_normal((2, 9 * f * f, H, W))).astype(np.float32)
    return flow, mask, float(f)


@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
def test_reference_forward_is_rafts_composition(geo, f):
    flow, mask, scale = _case(geo, f, seed=sum(geo) + f)
    ref, S, Sa, n = RU.forward(flow, mask, f, scale)
    got = RU.compose(torch.from_numpy(flow).double(), torch.from_numpy(mask).double(), f, scale).numpy()
    assert ref.shape == got.shape == (2, geo[2], f * geo[0], f * geo[1])
    assert np.abs(ref - got).max() < 1e-12, float(np.abs(ref - got).max())
    assert np.abs(ref).max() > 0.1 and (S >= np.abs(ref) - 1e-12).all() and (Sa >= 0).all()
    assert n.min() == (1 if geo[:2] == (1, 1) else 4) and n.max() == (1 if geo[:2] == (1, 1) else 9)


@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
def test_reference_gradients_are_autograd_through_the_composition(geo, f):
    flow, mask, scale = _case(geo, f, seed=sum(geo) + f + 1)
    go = np.random.default_rng(5).standard_normal((2, geo[2], f * geo[0], f * geo[1]))
    (gf, Sg, Sga, n), (gm, Bm0, Bm1) = RU.backward(flow, mask, go, f, scale)
    tf, tm = torch.from_numpy(flow).double().requires_grad_(True), torch.from_numpy(mask).double().requires_grad_(True)
    RU.compose(tf, tm, f, scale).backward(torch.from_numpy(go))
    assert np.abs(gf - tf.grad.numpy()).max() < 1e-10 and np.abs(gm - tm.grad.numpy()).max() < 1e-10
    assert np.abs(gf).max() > 0.1 and (Sg >= np.abs(gf) - 1e-10).all() and (Bm0 >= np.abs(gm) - 1e-10).all() and (Bm1 >= 0).all()
    if geo[:2] != (1, 1):
        assert np.abs(gm).max() > 0.01
    assert n.max() == (1 if geo[:2] == (1, 1) else 9) * f * f


def test_reference_one_hot_and_equal_logits_in_closed_form():
    """One tap 200 above the rest selects scale * flow at that neighbour (0 where it is outside the image); equal logits give
    the mean of the present neighbours over nine."""
    f, scale = 2, 3.0
    flow = np.arange(1.0, 13.0, dtype=np.float32).reshape(1, 2, 2, 3)
    H, W = 2, 3
    for k in range(9):
        mask = np.zeros((1, 9 * f * f, H, W), np.float32)
        mask[:, k * f * f:(k + 1) * f * f] = 200.0
        out, S, Sa, n = RU.forward(flow, mask, f, scale)
        for y in range(H):
            for x in range(W):
                yy, xx = y + k // 3 - 1, x + k % 3 - 1
                want = scale * flow[0, :, yy, xx] if 0 <= yy < H and 0 <= xx < W else np.zeros(2)
                blk = out[0, :, f * y:f * y + f, f * x:f * x + f]
                assert np.abs(blk - want[:, None, None]).max() <= 1e-80 * 40, (k, y, x)   # the other eight weigh e^-200 each
    # the sub-position picks its own tap: mask channel k f^2 + i f + j
    mask = np.zeros((1, 9 * f * f, H, W), np.float32)
    mask[0, 5 * f * f + 1 * f + 0, 0, 1] = 200.0      # tap (ky, kx) = (1, 2) for sub-row 1, sub-column 0 of pixel (0, 1)
    out = RU.forward(flow, mask, f, scale)[0]
    assert abs(out[0, 0, 1, 2] - scale * flow[0, 0, 0, 2]) < 1e-70 and abs(out[0, 1, 1, 2] - scale * flow[0, 1, 0, 2]) < 1e-70
    # equal logits: the mean over nine, absent taps counting as nothing
    out, S, Sa, n = RU.forward(flow, np.full((1, 9 * f * f, H, W), -7.0, np.float32), f, scale)
    pad = np.zeros((2, H + 2, W + 2))
    pad[:, 1:-1, 1:-1] = flow[0]
    for y in range(H):
        for x in range(W):
            want = scale * pad[:, y:y + 3, x:x + 3].sum((1, 2)) / 9
            assert np.abs(out[0, :, f * y:f * y + f, f * x:f * x + f] - want[:, None, None]).max() < 1e-12
    assert (Sa == 0).all() and n[0, 0, 0, 0] == 4 and n[0, 0, 1, 3] == 6
    # the gradient of equal logits with gO = 1 on one channel: p_k (v_k - mean), summing to 0 over k also where taps are absent
    go = np.zeros((1, 2, f * H, f * W))
    go[0, 0] = 1.0
    (gf, _, _, nf), (gm, _, _) = RU.backward(flow, np.zeros((1, 9 * f * f, H, W), np.float32), go, f, scale)
    assert np.abs(gm.reshape(1, 9, f * f, H, W).sum(1)).max() < 1e-12
    assert abs(gm[0, 0, 0, 0] - (0.0 - scale * (1 + 2 + 4 + 5) / 9) / 9) < 1e-12     # tap 0 of pixel (0, 0) is absent: d = 0
    # grad_flow: every pixel receives scale * f^2 / 9 from each of its neighbours inside the image, itself included
    assert np.allclose(gf[0, 0], scale * f * f / 9 * np.array([[4, 6, 4], [4, 6, 4]]), atol=1e-12) and (gf[0, 1] == 0).all()
    assert nf[0, 0].tolist() == [[16, 24, 16], [16, 24, 16]]


def test_kernels_use_no_scratch_and_fit_the_lds(tmp_path):
    """0 bytes of scratch and at most 60 KB of LDS for every instantiation: forward and grad_mask kernels for 3 factors x
    4 channel counts x 3 mask types, and the grad_flow gather; device code only, the library's own flags."""
    import build
    src = os.path.join(PKG, "csrc", "convex_upsample.hip")
    r = subprocess.run([build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "convex_upsample.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S*convex_upsample_\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", r.stderr, flags=re.S)
    names = [k for k, _, _ in kernels]
    per = 3 * RU.header_macros()["FN2U_MAX_CHANNELS"] * 3
    assert sum("convex_upsample_fwd" in k for k in names) == per, names
    assert sum("convex_upsample_bwd_mask" in k for k in names) == per, names
    assert sum("convex_upsample_bwd_flow" in k for k in names) == 1 and len(names) == 2 * per + 1, names
    for name, body, lds in kernels:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
        assert scratch == 0, f"{name} spills {scratch} bytes per lane"
        assert int(lds) <= 60 * 1024, f"{name} uses {lds} bytes of LDS"
