"""CPU-side checks of ForwardWarp's library (include/flownet2_hip_splat.h, libflownet2_hip_splat.so; what it exports and
links is in tests/test_libraries_host.py): its workspace size, the five headers in one translation unit, every rejection in front of a launch (host
pointers, no GPU), the refusals at the Python doors, the float64 reference against the PyTorch composition (values and both
gradients) and in closed form, the tap computation (csrc/splat_taps.h) as a stand-alone program under the undefined-behaviour
sanitizer, and the kernels' scratch and LDS budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import forward_warp_ref as RS
import fn2_capi

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4


def test_workspace_bytes():
    ws = fn2_capi.splat_lib().fn2s_forward_warp_forward_det_workspace_bytes
    # the plane maxima, 4 bytes each and rounded up to 256, then one int64 per element
    assert ws(8, 32, 96, 128) == 1024 + 8 * 8 * 32 * 96 * 128
    assert ws(2, 3, 5, 7) == 256 + 8 * 2 * 3 * 5 * 7 and ws(1, 1, 1, 1) == 256 + 8 and ws(1, 65, 1, 1) == 512 + 8 * 65
    for bad in ((0, 2, 4, 4), (-1, 2, 4, 4), (1, 0, 4, 4), (1, 2, 0, 4), (1, 2, 4, 0), (1, 2, 65536, 32768), (65536, 32768, 1, 1),
                (1 << 12, 1 << 12, 1 << 12, 1 << 12)):
        assert ws(*bad) == 0, bad


def test_five_headers_in_one_translation_unit(tmp_path):
    """The splat header restates the codes unless one of the other four came first."""
    a, x, l, u, s = "flownet2_hip.h", "flownet2_hip_ext.h", "flownet2_hip_lookup.h", "flownet2_hip_upsample.h", "flownet2_hip_splat.h"
    for i, incs in enumerate(((a, x, l, u, s), (x, l, u, s), (a, l, u, s), (a, x, u, s), (a, x, l, s), (l, u, s), (u, s), (l, s), (x, s),
                              (a, s), (s,), (s, s))):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in incs) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2S_TILED + FN2S_HALO + FN2S_K_I + FN2S_K_F];\n"
                       "size_t (*ws)(int, int, int, int) = fn2s_forward_warp_forward_det_workspace_bytes;\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.splat_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis1 = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    mis2 = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    mis4 = ctypes.c_void_p(ctypes.addressof(buf) + 4)     # aligned for a float, not for the int64 workspace
    shape = (1, 2, 8, 16)
    need = lib.fn2s_forward_warp_forward_det_workspace_bytes(*shape)

    def fwd(ptrs, shp, algo=0):
        return lib.fn2s_forward_warp_forward(*ptrs, *shp, algo, null)

    def det(ptrs, shp, nbytes=1 << 40):
        return lib.fn2s_forward_warp_forward_det(*ptrs, nbytes, *shp, null)

    def bwd(ptrs, shp):
        return lib.fn2s_forward_warp_backward(*ptrs, *shp, null)

    # (call, number of pointers, pointers that must not be NULL)
    for call, n, required in ((fwd, 3, (0, 1, 2)), (det, 4, (0, 1, 2, 3)), (bwd, 5, (0, 1, 2))):
        good = [p] * n
        # 1. sizes, whatever else is wrong
        for shp in ((-1, 2, 8, 16), (1, 0, 8, 16), (1, -2, 8, 16), (1, 2, 0, 16), (1, 2, 8, 0), (1, 2, -8, 16), (0, 0, 8, 16)):
            assert call([null] * n, shp) == EINVAL, shp
        # 2. a plane of 2^31 elements, 2^31 planes, 2^48 elements, 2^31 workgroups
        for shp in ((1, 1, 65536, 32768), (0, 1, 65536, 32768), (65536, 32768, 1, 1), (1 << 12, 1 << 12, 1 << 12, 1 << 12),
                    (1 << 24, 1, 1, 1 << 15)):
            assert call([null] * n, shp) == EUNSUPPORTED, shp
        assert call([null] * n, (1, 1, 32768, 65535)) == EINVAL      # just below 2^31: accepted, the NULL pointers are next
        # 3. an empty batch: nothing to do, whatever the pointers
        assert call([null] * n, (0,) + shape[1:]) == OK
        assert call([mis1] * n, (0,) + shape[1:]) == OK
        # 4. NULL pointers, also next to a misaligned one: NULL is reported first
        for i in required:
            ptrs = list(good)
            ptrs[i] = null
            ptrs[(i + 1) % 3] = mis1
            assert call(ptrs, shape) == EINVAL, i
        # 5. alignment
        for i in range(n):
            for mis in (mis1, mis2):
                ptrs = list(good)
                ptrs[i] = mis
                assert call(ptrs, shape) == EALIGN, i
    # the backward: either gradient may be NULL, not both; a misaligned one is reported next to a NULL one
    assert bwd([p, p, p, null, null], shape) == EINVAL
    assert bwd([p, p, p, mis2, null], shape) == EALIGN and bwd([p, p, p, null, mis2], shape) == EALIGN
    # the deterministic forward: the workspace is aligned to 8 bytes, then measured
    assert det([p, p, p, mis4], shape) == EALIGN
    assert det([p, p, p, mis4], shape, 0) == EALIGN
    for nbytes in (0, 8, need - 1):
        assert det([p, p, p, p], shape, nbytes) == EINVAL, nbytes
    # the selector last of all
    for algo in (-1, 3, 100):
        assert fwd([p, p, p], shape, algo) == EINVAL
        assert fwd([p, p, mis1], shape, algo) == EALIGN
        assert fwd([p, p, p], (0,) + shape[1:], algo) == OK
    with pytest.raises(RuntimeError):
        fn2_capi.check(EUNSUPPORTED, "fn2s_forward_warp_forward")


def test_cpu_tensors_and_bad_arguments_are_refused():
    import forward_warp_cuda
    from networks.splat_package import ForwardWarp, ForwardWarpFunction, range_map, softsplat
    x, fl = torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 4, 5)
    e = torch.zeros(0)
    doors = (lambda a, f: forward_warp_cuda.forward(a, f, e, 0),
             lambda a, f: forward_warp_cuda.backward(a, f, torch.zeros(2, 3, 4, 5), e, e.clone()),
             lambda a, f: forward_warp_cuda.forward_alloc(a, f),
             lambda a, f: forward_warp_cuda.backward_alloc(a, f, torch.zeros(2, 3, 4, 5)),
             lambda a, f: forward_warp_cuda.apply(a, f),
             lambda a, f: ForwardWarpFunction.apply(a, f),
             lambda a, f: ForwardWarp()(a, f),
             lambda a, f: softsplat(a, f),
             lambda a, f: softsplat(a, f, mode="avg"),
             lambda a, f: softsplat(a, f, torch.zeros(a.shape[0], 1, 4, 5, dtype=a.dtype) if a.dim() == 4 else torch.zeros(1), mode="soft"))
    for door in doors:
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            door(x, fl)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        range_map(fl)
    # bad arguments are reported as such on any device, at every door
    for door in doors[:8]:
        for bad in (torch.zeros(2, 3, 4, 5), torch.zeros(2, 1, 4, 5)):
            with pytest.raises(RuntimeError, match="channels, expected 2"):
                door(x, bad)
        for shp in ((1, 2, 4, 5), (2, 2, 5, 5), (2, 2, 4, 6)):
            with pytest.raises(RuntimeError, match="must have the batch size, height and width of input"):
                door(x, torch.zeros(shp))
        with pytest.raises(RuntimeError, match="4-D"):
            door(x[0], fl)
        for t16 in (torch.float16, torch.bfloat16):
            with pytest.raises(RuntimeError, match=r"input must be float32.*\.float\(\).*round at every add"):
                door(x.to(t16), fl)
            with pytest.raises(RuntimeError, match=r"flow must be float32.*\.float\(\)"):
                door(x, fl.to(t16))
        with pytest.raises(RuntimeError, match=r"input must be float32, got Double.*\.float\(\)"):
            door(x.double(), fl)
    with pytest.raises(RuntimeError, match="algo 3 is not"):
        forward_warp_cuda.forward_alloc(x, fl, 3)
    with pytest.raises(RuntimeError, match="neither gradient"):
        forward_warp_cuda.backward_alloc(x, fl, x, False, False)
    with pytest.raises(ValueError, match="not one of"):
        softsplat(x, fl, mode="max")
    for mode in ("linear", "soft"):
        with pytest.raises(ValueError, match="needs a metric"):
            softsplat(x, fl, mode=mode)
        with pytest.raises(ValueError, match="must be N x 1 x H x W"):
            softsplat(x, fl, torch.zeros(2, 2, 4, 5), mode=mode)
    for mode in ("sum", "avg"):
        with pytest.raises(ValueError, match="takes no metric"):
            softsplat(x, fl, torch.zeros(2, 1, 4, 5), mode=mode)
    with pytest.raises(ValueError, match="N x 2 x H x W"):
        range_map(fl[0])
    assert (forward_warp_cuda.AUTO, forward_warp_cuda.GENERAL, forward_warp_cuda.TILED) == (0, 1, 2)
    assert (fn2_capi.FN2S_AUTO, fn2_capi.FN2S_GENERAL, fn2_capi.FN2S_TILED) == (0, 1, 2)


def _exact_case():
    """2 x 3 x 5 x 7, a smooth fractional flow on a grid of 2^-10: x + flow, ax and 1 - ax are then exact in fp32 and in
    float64 alike, so the reference's fp32 taps and the composition's float64 taps are the same numbers."""
    rng = np.random.default_rng(3)
    inp = rng.standard_normal((2, 3, 5, 7)).astype(np.float32)
    flow = np.array([1.25, -0.75])[None, :, None, None] + 0.4 * rng.standard_normal((2, 2, 5, 7))
    flow = (np.rint(flow * 1024) / 1024).astype(np.float32)
    return inp, flow


def test_reference_is_the_index_put_composition():
    inp, flow = _exact_case()
    go = np.random.default_rng(4).standard_normal(inp.shape)
    out, S, n = RS.forward(inp, flow)
    (gi, Si), (gf, Sf) = RS.backward(inp, flow, go)
    ti, tf = torch.from_numpy(inp).double().requires_grad_(True), torch.from_numpy(flow).double().requires_grad_(True)
    got = RS.compose(ti, tf)
    got.backward(torch.from_numpy(go))

    def rel(a, b):
        return float(np.abs(a - b).max() / np.abs(b).max())

    assert rel(out, got.detach().numpy()) < 1e-12 and rel(gi, ti.grad.numpy()) < 1e-12 and rel(gf, tf.grad.numpy()) < 1e-12
    assert np.abs(out).max() > 0.5 and np.abs(gi).max() > 0.5 and np.abs(gf).max() > 0.5
    assert (S >= np.abs(out) - 1e-12).all() and (Si >= np.abs(gi) - 1e-12).all() and (Sf >= np.abs(gf) - 1e-12).all()
    assert n.max() >= 4 and n.min() == 0 and 0.5 < RS.inside_share(flow) < 1.0     # some pixels leave the image
    # the fixed-point result is the same sum, to the precision of float32
    assert (np.abs(RS.forward_fixed(inp, flow) - out) <= 2.0 ** -22 * S + 1e-30).all()


def test_reference_closed_forms():
    rng = np.random.default_rng(5)
    inp = rng.standard_normal((2, 3, 5, 7)).astype(np.float32)
    # zero flow is the identity
    out, S, n = RS.forward(inp, RS.flow_family("zero", 2, 5, 7))
    assert (out == inp).all() and (n == 1).all() and (RS.forward_fixed(inp, np.zeros((2, 2, 5, 7), np.float32)) == inp).all()
    # an integer shift is a shift: (3, -2) moves column x to x + 3 and row y to y - 2
    out, S, n = RS.forward(inp, RS.flow_family("shift", 2, 5, 7))
    want = np.zeros_like(out)
    want[:, :, :3, 3:] = inp[:, :, 2:, :4]
    assert (out == want).all() and (n[:, :, :3, 3:] == 1).all() and n.sum() == 2 * 3 * 3 * 4
    go = rng.standard_normal(inp.shape)
    (gi, _), (gf, _) = RS.backward(inp, RS.flow_family("shift", 2, 5, 7), go)
    wantg = np.zeros_like(gi)
    wantg[:, :, 2:, :4] = go[:, :, :3, 3:]
    assert (gi == wantg).all()
    # half a pixel to the right: two taps of 1/2 each; the gradient in x is the difference of the two taps' gO
    flow = np.zeros((1, 2, 1, 4), np.float32)
    flow[:, 0] = 0.5
    one = np.ones((1, 1, 1, 4), np.float32)
    out, S, n = RS.forward(one, flow)
    assert out[0, 0, 0].tolist() == [0.5, 1.0, 1.0, 1.0] and n[0, 0, 0].tolist() == [1, 2, 2, 2]
    go = np.array([1.0, 2.0, 4.0, 8.0]).reshape(1, 1, 1, 4)
    (gi, _), (gf, _) = RS.backward(one, flow, go)
    assert gi[0, 0, 0].tolist() == [1.5, 3.0, 6.0, 4.0] and gf[0, 0, 0].tolist() == [1.0, 2.0, 4.0, -8.0] and (gf[0, 1] == -gi[0, 0]).all()
    # every pixel onto one point: the fullest cell has n = H W
    flow = RS.flow_family("converge", 2, 5, 7)
    out, S, n = RS.forward(inp, flow)
    assert n.max() == 35 and n[0, 0, 2, 3] == 35 and np.count_nonzero(n[0, 0]) == 4
    assert abs(out[1, 2, 2, 3] - 0.5 * 0.75 * inp[1, 2].astype(np.float64).sum()) < 1e-12
    # a broken plane and a zero plane in the fixed-point contract
    bad = inp.copy()
    bad[0, 1, 2, 2] = np.inf
    bad[1, 0] = 0
    fx = RS.forward_fixed(bad, flow)
    good = RS.forward_fixed(inp, flow)
    assert np.isnan(fx[0, 1]).all() and (fx[1, 0] == 0).all() and not np.signbit(fx[1, 0]).any()
    keep = np.ones((2, 3), bool)
    keep[0, 1] = keep[1, 0] = False
    assert (fx[keep] == good[keep]).all()


# positions along one axis of n cells, as (coordinate, flow): -1 and n exactly, the floats just inside both, NaN, +-inf,
# +-1e30, -0.0, and 2^24 + 1 (not a float: the coordinate's own conversion rounds it)
_TAPS_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "splat_taps.h"
int main()
{
    int n, i;
    unsigned bits;
    while (std::scanf("%d %d %x", &n, &i, &bits) == 3) {
        float fl;
        std::memcpy(&fl, &bits, 4);
        const float f = splat_pos(i, fl);
        const SplatTaps a = splat_taps(f, 0.0f, n, 1), b = splat_taps(0.0f, f, 1, n);
        std::printf("%d %d %a %a %a %a %a %a | %d %d %a %a %a %a %a %a\n", a.valid, a.x0, a.ax, a.bx, a.w00, a.w01, a.w10, a.w11, b.valid, b.y0,
                    b.ay, b.by, b.w00, b.w01, b.w10, b.w11);
    }
    return 0;
}
"""


def test_taps_program_under_the_undefined_behaviour_sanitizer(tmp_path):
    """csrc/splat_taps.h in a stand-alone program: a float-to-int conversion of an out-of-range value, made before the validity
    test, would stop it here (float-cast-overflow, no recovery).  Its output is the reference's."""
    src, exe = tmp_path / "taps.cpp", tmp_path / "taps"
    src.write_text(_TAPS_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                        "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    f32 = np.float32
    below = lambda v: np.nextafter(f32(v), f32(-np.inf))     # noqa: E731
    above = lambda v: np.nextafter(f32(v), f32(np.inf))      # noqa: E731
    cases = []      # (n, coordinate, flow)
    for n in (7, 1, 130):
        cases += [(n, 3 % n, f32(-1 - 3 % n)), (n, 0, f32(n)), (n, 0, below(n)), (n, 0, above(-1)), (n, 0, f32(np.nan)), (n, 0, f32(np.inf)),
                  (n, 0, f32(-np.inf)), (n, n - 1, f32(1e30)), (n, n - 1, f32(-1e30)), (n, 0, f32(-0.0)), (n, 0, f32(0.0)), (n, n - 1, f32(0.25)),
                  (n, 0, f32(-0.75)), (n, n - 1, f32(-1e-30)), (n, 0, f32(3e9)), (n, 0, f32(-3e9))]
    big = 1 << 25
    cases += [(big, (1 << 24) + 1, f32(0)), (big, (1 << 24) + 1, f32(1)), (big, (1 << 24) + 3, f32(-0.0)), (big, big - 1, f32(0)),
              (big, big - 1, f32(2)), (2147483647, 2147483647 - 64, f32(0)), (2147483647, 2147483647, f32(-200))]
    text = "".join("%d %d %08x\n" % (n, i, int(np.asarray(fl, f32).view(np.uint32))) for n, i, fl in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    seen_valid = seen_invalid = 0
    for (n, i, fl), line in zip(cases, lines):
        for axis, half in enumerate(line.split("|")):
            tok = half.split()
            got = [int(tok[0]), int(tok[1])] + [float.fromhex(t) for t in tok[2:]]
            # the reference on a 1 x n (or n x 1) image whose pixel i carries the flow
            flow = np.zeros((1, 2, 1, 1), f32)
            with np.errstate(invalid="ignore", over="ignore"):
                pos = f32(f32(i) + fl)
            valid = bool(pos > -1) and bool(pos < f32(n))
            if valid:
                x0 = int(np.floor(pos))
                a = f32(pos - np.floor(pos))
                b = f32(f32(1) - a)
                w = [b, a, f32(0), f32(0)] if axis == 0 else [b, f32(0), a, f32(0)]      # the other axis sits at 0: its a = 0, b = 1
                want = [1, x0, float(a), float(b)] + [float(v) for v in w]
                assert -1 <= x0 <= n - 1
                seen_valid += 1
            else:
                want = [0, 0] + [0.0] * 6
                seen_invalid += 1
            assert got == want, (n, i, fl, axis, got, want)
            del flow
    assert seen_valid >= 40 and seen_invalid >= 40
    # and the reference's own taps say the same of pixel 0 of seven rows: -1 and n are outside, the floats next to them inside
    flow = np.zeros((7, 2, 1, 7), f32)
    flow[:, 0, 0, 0] = [-1, above(-1), 7, below(7), np.nan, np.inf, -1e30]
    t = RS.taps(flow)
    assert t["valid"][:, 0, 0].tolist() == [False, True, False, True, False, False, False]
    assert t["x0"][:, 0, 0].tolist() == [0, -1, 0, 6, 0, 0, 0]


def test_kernels_use_no_scratch_and_fit_the_lds(tmp_path):
    """0 bytes of scratch for every instantiation -- general and deterministic forward, tiled forward, plane maxima, conversion,
    three backward forms -- and the tiled kernel's LDS is the patch DESIGN 4.13 states: FN2S_CHANNEL_GROUP channels of
    (FN2S_TILE_H + 2 FN2S_HALO) x (FN2S_TILE_W + 2 FN2S_HALO + 1) fp64 cells, within 32 KB; device code only, the library's own flags."""
    import build
    src = os.path.join(PKG, "csrc", "forward_warp.hip")
    r = subprocess.run([build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "forward_warp.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S*splat_\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", r.stderr, flags=re.S)
    names = [k for k, _, _ in kernels]
    for part, count in (("splat_fwd_general", 2), ("splat_fwd_tiled", 1), ("splat_plane_max", 1), ("splat_convert", 1), ("splat_bwd", 3)):
        assert sum(part in k for k in names) == count, (part, names)
    assert len(names) == 8, names
    m = RS.header_macros()
    patch = 8 * m["FN2S_CHANNEL_GROUP"] * (m["FN2S_TILE_H"] + 2 * m["FN2S_HALO"]) * (m["FN2S_TILE_W"] + 2 * m["FN2S_HALO"] + 1)
    assert patch <= 32 * 1024
    for name, body, lds in kernels:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
        assert scratch == 0, f"{name} spills {scratch} bytes per lane"
        want = patch if "splat_fwd_tiled" in name else 16 if "splat_plane_max" in name else 0
        assert int(lds) == want, f"{name} uses {lds} bytes of LDS, expected {want}"


# ------------------------------------------------------------------ the input families
_FAMILY_SHAPES = ((1, 2, 17, 67), (2, 5, 33, 130))


def _ratio(err, bound):
    return float((np.abs(err) / bound).max())


def test_input_families_keep_their_conditions():
    """Every family asserts in ``input_family`` what it is for, at both shapes the GPU tests use; the standard normal input
    meets none of the conditions of ``cancel``, ``subnormal`` and ``huge``."""
    for shape in _FAMILY_SHAPES:
        B, C, H, W = shape
        for name in RS.INPUT_FAMILIES:
            inp, go = RS.input_family(name, shape, 5)
            assert inp.shape == go.shape == shape and inp.dtype == go.dtype == np.float32
            assert set(RS.FAMILY_FLOWS[name]) <= {"smooth", "converge", "shift", "zero"}
        inp, _ = RS.input_family("normal", shape, 5)
        out, S, n = RS.forward(inp, RS.flow_family("converge", B, H, W))
        full = n == H * W
        assert full.any() and not (np.abs(out[full]) <= 2.0 ** -6 * S[full]).all()
        assert np.abs(inp).min() > 2.0 ** -120 and np.abs(inp).max() < 2.0 ** 125
    graded, go = RS.input_family("graded", _FAMILY_SHAPES[1], 5)
    tops = np.log2(np.abs(graded.astype(np.float64)).max(axis=(2, 3))).ravel()
    assert all(abs(t - e) < 3 for t, e in zip(tops, RS.GRADED_EXPONENTS * 2))
    assert "converge" not in RS.FAMILY_FLOWS["huge"]


def test_emulation_stays_inside_the_bounds_on_every_family():
    """The atomic forward and both gradients, emulated in numpy float32 from the header's operation list, stay inside the
    header's bounds on every input family and flow, and the fixed-point result inside the forward bound plus 2^(K - 62) M per
    contribution; the worst error / bound per family is printed.  The gradients of ``huge`` overflow and are not asked for."""
    m = RS.header_macros()
    for name in RS.INPUT_FAMILIES:
        worst = np.zeros(4)
        for shape in _FAMILY_SHAPES:
            B, C, H, W = shape
            inp, go = RS.input_family(name, shape, 50 + H)
            for fl in RS.FAMILY_FLOWS[name]:
                flow = RS.flow_family(fl, B, H, W)
                out, S, n = RS.forward(inp, flow)
                r = [_ratio(RS.emulate_forward(inp, flow) - out, RS.forward_bound(S, n)), _ratio(RS.forward_fixed(inp, flow) - out, RS.fixed_bound(inp, S, n)), 0, 0]
                if name != "huge":
                    (gi, Si), (gf, Sf) = RS.backward(inp, flow, go)
                    egi, egf = RS.emulate_backward(inp, flow, go)
                    r[2] = _ratio(egi - gi, m["FN2S_K_I"] * (RS.U23 * Si + RS.SUB))
                    r[3] = _ratio(egf - gf, (C + m["FN2S_K_F"]) * (RS.U23 * Sf + RS.SUB))
                worst = np.maximum(worst, r)
        print(f"emulation, {name}: forward {worst[0]:.3f}, fixed point {worst[1]:.3f}, grad_input {worst[2]:.3f}, grad_flow {worst[3]:.3f}")
        assert worst.max() <= 1.0, (name, worst)


def test_planted_mistakes_pass_the_normal_input_and_fail_a_new_family():
    """Teeth.  An addition that flushes a subnormal sum to 0 stays inside the forward bound on the standard normal input and
    leaves it on ``subnormal``; a fixed-point scaling done in float32 (2^s a float32 of its own) gives the contract's bits on the
    standard normal input, where s is about 47, and not on ``graded`` (s = 150 for the plane of 2^-100) nor on ``subnormal``."""
    shape = _FAMILY_SHAPES[0]
    B, C, H, W = shape
    flow = RS.flow_family("smooth", B, H, W)
    seen = {}
    for name in ("normal", "subnormal", "graded"):
        inp, _ = RS.input_family(name, shape, 50 + H)
        out, S, n = RS.forward(inp, flow)
        if name != "graded":
            seen[name, "ftz_add"] = _ratio(RS.emulate_forward(inp, flow, "ftz_add") - out, RS.forward_bound(S, n))
        seen[name, "float_scale"] = bool((RS.forward_fixed(inp, flow, "float_scale").view(np.uint32) == RS.forward_fixed(inp, flow).view(np.uint32)).all())
    print(seen)
    assert seen["normal", "ftz_add"] <= 1.0 < seen["subnormal", "ftz_add"]
    assert seen["normal", "float_scale"] and not seen["graded", "float_scale"] and not seen["subnormal", "float_scale"]
