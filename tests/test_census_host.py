"""CPU-side checks of the census library (include/flownet2_hip_census.h, libflownet2_hip_census.so; what it exports and links
is in tests/test_libraries_host.py): the six headers in one translation unit, every rejection in front of a launch (host pointers,
no GPU), the refusals at the Python doors, the float64 reference against the PyTorch composition (values and both gradients) and
in closed form, the arithmetic header (csrc/census_arith.h) as a stand-alone program under the undefined-behaviour sanitizer, and
the kernels' scratch and LDS budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import census_ref as RC
import fn2_capi

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
U = 2.0 ** -24


def test_six_headers_in_one_translation_unit(tmp_path):
    """The census header restates the codes unless one of the other five came first."""
    a, x, l, u, s, c = ("flownet2_hip.h", "flownet2_hip_ext.h", "flownet2_hip_lookup.h", "flownet2_hip_upsample.h", "flownet2_hip_splat.h",
                        "flownet2_hip_census.h")
    for i, incs in enumerate(((a, x, l, u, s, c), (x, l, u, s, c), (a, l, u, s, c), (a, x, u, s, c), (a, x, l, s, c), (a, x, l, u, c),
                              (l, u, s, c), (u, s, c), (s, c), (u, c), (l, c), (x, c), (a, c), (c,), (c, c))):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in incs) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2C_TILE_H + FN2C_PAD + FN2C_MAX_DISTANCE - FN2C_FWD_BOUND_LOG2\n"
                       "          - FN2C_BWD_BOUND_LOG2];\n"
                       "char lds[FN2C_LDS_BYTES(3, FN2C_MAX_DISTANCE) == 18744 && FN2C_LDS_BYTES(2, 3) == 12496 ? 1 : -1];\n"
                       "int (*fwd)(const void *, const void *, void *, int, int, int, int, int, float, int, void *) = fn2c_census_forward;\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.census_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis1 = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    mis2 = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    shape = (1, 3, 8, 16)

    def fwd(ptrs, shp, md=3, scale=255.0, normalize=1):
        return lib.fn2c_census_forward(*ptrs, *shp, md, scale, normalize, null)

    def bwd(ptrs, shp, md=3, scale=255.0, normalize=1):
        return lib.fn2c_census_backward(*ptrs, *shp, md, scale, normalize, null)

    # (call, number of pointers, pointers that must not be NULL)
    for call, n, required in ((fwd, 3, (0, 1, 2)), (bwd, 5, (0, 1, 2))):
        good = [p] * n
        # 1. sizes, whatever else is wrong (NULL pointers, a max_distance out of range)
        for shp in ((-1, 3, 8, 16), (1, 0, 8, 16), (1, -2, 8, 16), (1, 3, 0, 16), (1, 3, 8, 0), (1, 3, -8, 16), (0, 0, 8, 16)):
            assert call([null] * n, shp, md=0) == EINVAL, shp
        # 2. a plane of 2^31 elements, 2^31 planes, 2^48 elements, 2^31 workgroups -- also with a channel count that is refused later
        for shp in ((1, 1, 65536, 32768), (0, 1, 65536, 32768), (65536, 32768, 1, 1), (1 << 12, 1 << 12, 1 << 12, 1 << 12),
                    (1 << 24, 1, 1, 1 << 15)):
            assert call([null] * n, shp, md=4) == EUNSUPPORTED, shp
        assert call([null] * n, (1, 1, 32768, 65535)) == EINVAL      # just below 2^31: accepted, the NULL pointers are next
        # 3. an empty batch: nothing to do, whatever the pointers and the parameters
        assert call([null] * n, (0,) + shape[1:]) == OK
        assert call([mis1] * n, (0, 2, 8, 16), md=7) == OK
        # 4. NULL pointers, also next to a misaligned one: NULL is reported first
        for i in required:
            ptrs = list(good)
            ptrs[i] = null
            ptrs[(i + 1) % 3] = mis1
            assert call(ptrs, shape) == EINVAL, i
        # 5. alignment, in front of the parameters
        for i in range(n):
            for mis in (mis1, mis2):
                ptrs = list(good)
                ptrs[i] = mis
                assert call(ptrs, shape, md=0) == EALIGN, i
        # 6. the parameters last of all: the channel count, max_distance, a scale that is not a finite number
        for C in (2, 4, 64):
            assert call(good, (1, C, 8, 16)) == EINVAL, C
        for md in (0, 4, -1, 100):
            assert call(good, shape, md=md) == EINVAL, md
            assert call(good[:-1] + [mis2], shape, md=md) == EALIGN
            assert call(good, (0,) + shape[1:], md=md) == OK
        for scale in (float("nan"), float("inf"), -float("inf")):
            assert call(good, shape, scale=scale) == EINVAL, scale
    # the backward: either gradient may be NULL, not both; a misaligned one is reported next to a NULL one
    assert bwd([p, p, p, null, null], shape) == EINVAL
    assert bwd([p, p, p, mis2, null], shape) == EALIGN and bwd([p, p, p, null, mis2], shape) == EALIGN
    assert bwd([p, p, p, null, null], shape, md=4) == EINVAL
    with pytest.raises(RuntimeError):
        fn2_capi.check(EUNSUPPORTED, "fn2c_census_forward")


def test_cpu_tensors_and_bad_arguments_are_refused():
    import census_cuda
    from networks.census_package import CensusFunction, CensusLoss, TernaryCensus, census_distance
    x, y = torch.zeros(2, 3, 8, 9), torch.zeros(2, 3, 8, 9)
    e = torch.zeros(0)
    go = torch.zeros(2, 1, 8, 9)
    doors = (lambda a, b, md=3: census_cuda.forward(a, b, e, md),
             lambda a, b, md=3: census_cuda.backward(a, b, go, e, e.clone(), md),
             lambda a, b, md=3: census_cuda.forward_alloc(a, b, md),
             lambda a, b, md=3: census_cuda.backward_alloc(a, b, go, md),
             lambda a, b, md=3: census_cuda.apply(a, b, md),
             lambda a, b, md=3: CensusFunction.apply(a, b, md),
             lambda a, b, md=3: census_distance(a, b, md),
             lambda a, b, md=3: census_distance(a, b, max_distance=md, scale=1.0, normalize=False),
             lambda a, b, md=3: TernaryCensus(3)(a, b) if md == 3 else census_distance(a, b, md),
             lambda a, b, md=3: CensusLoss(3)(a, b) if md == 3 else census_distance(a, b, md))
    for door in doors:
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            door(x, y)
        # bad arguments are reported as such on any device, at every door
        for shp in ((1, 3, 8, 9), (2, 1, 8, 9), (2, 3, 9, 9), (2, 3, 8, 8)):
            with pytest.raises(RuntimeError, match="must have the shape of im1"):
                door(x, torch.zeros(shp))
        for C in (2, 4):
            with pytest.raises(RuntimeError, match="channels, expected 1"):
                door(torch.zeros(2, C, 8, 9), torch.zeros(2, C, 8, 9))
        with pytest.raises(RuntimeError, match="4-D"):
            door(x[0], y[0])
        for dt, name in ((torch.float16, "Half"), (torch.bfloat16, "BFloat16"), (torch.float64, "Double")):
            with pytest.raises(RuntimeError, match=rf"im1 must be float32, got {name}.*\.float\(\)"):
                door(x.to(dt), y)
            with pytest.raises(RuntimeError, match=rf"im2 must be float32, got {name}.*\.float\(\)"):
                door(x, y.to(dt))
        for md in (0, 4, -1):
            with pytest.raises(RuntimeError, match=f"max_distance {md} is not 1, 2 or 3"):
                door(x, y, md)
    with pytest.raises(RuntimeError, match="scale .* is not a finite float"):
        census_cuda.forward_alloc(x, y, 3, float("inf"))
    with pytest.raises(RuntimeError, match="neither gradient"):
        census_cuda.backward_alloc(x, y, go, 3, 255.0, True, False, False)
    for md in (0, 4):
        with pytest.raises(ValueError, match="is not 1, 2 or 3"):
            TernaryCensus(md)
        with pytest.raises(ValueError, match="is not 1, 2 or 3"):
            CensusLoss(md)
    assert census_cuda.MAX_DISTANCE == 3 == RC.header_macros()["FN2C_MAX_DISTANCE"]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("md,normalize", [(1, True), (2, False), (3, True), (3, False)])
def test_reference_is_the_conv2d_composition(C, md, normalize):
    """Values and both gradients of the float64 reference against autograd of the composition in float64, from the same fp32 grey
    intensities, to 1e-12 relative; the channel weights of the image gradient on top."""
    shape = (2, C, 11, 13)
    im1, im2, go = RC.image_pair(shape, 100 + 10 * md + C)
    g1, g2 = RC.grey(im1, 255.0), RC.grey(im2, 255.0)
    out = RC.forward(im1, im2, md, 255.0, normalize)
    a1, a2, Ag = RC.backward_grey(g1, g2, go, md, normalize)
    t1, t2 = (torch.from_numpy(g.astype(np.float64))[:, None].requires_grad_(True) for g in (g1, g2))
    got = RC.compose_grey(t1, t2, md, normalize)
    got.backward(torch.from_numpy(go.astype(np.float64)))

    def rel(a, b):
        return float(np.abs(a - b).max() / np.abs(b).max())

    assert rel(out, got.detach().numpy()) <= 1e-12
    assert rel(a1, t1.grad.numpy()[:, 0]) <= 1e-12 and rel(a2, t2.grad.numpy()[:, 0]) <= 1e-12
    w = RC.weight(md, normalize) * (2 * md + 1) ** 2
    assert out.max() > 0.02 * w and np.abs(a1).max() > 1e-4 * w and np.abs(a2).max() > 1e-4 * w     # not trivially small
    assert (Ag >= np.abs(a1) / 2.4).all() and (Ag >= np.abs(a2) / 2.4).all()          # |h' f'| <= 2.06 * 1.12
    gi1, gi2, A = RC.backward(im1, im2, go, md, 255.0, normalize)
    cw = [1.0] if C == 1 else [float(c) for c in RC.CW]
    for c in range(C):
        assert np.array_equal(gi1[:, c], cw[c] * 255.0 * a1) and np.array_equal(gi2[:, c], cw[c] * 255.0 * a2)
        assert np.array_equal(A[:, c], cw[c] * 255.0 * Ag)
    # the composition from the images themselves, in fp32: the family's error stays far inside the bound
    o32 = RC.compose(torch.from_numpy(im1), torch.from_numpy(im2), md, 255.0, normalize).numpy().astype(np.float64)
    assert np.abs(o32 - out).max() <= RC.forward_bound(md, normalize) / 4


def test_reference_closed_forms():
    rng = np.random.default_rng(5)
    for C, md in ((1, 1), (3, 2), (3, 3), (1, 3)):
        shape = (2, C, 12, 15)
        im1, im2, go = RC.image_pair(shape, 7 + md)
        # identical images: distance 0 and zero gradients
        out = RC.forward(im1, im1, md)
        g1, g2, A = RC.backward(im1, im1, go, md)
        assert (out == 0).all() and (g1 == 0).all() and (g2 == 0).all() and A.max() > 0
        # census is brightness-invariant: a constant added to the grey plane changes nothing.  On grey planes that hold
        # integers the sum is exact in fp32.
        ga = np.rint(RC.grey(im1, 255.0)).astype(np.float32)
        assert (RC.forward_grey(ga, ga + np.float32(17), md) == 0).all()
        # the border ring is exactly 0, and gO on the ring reaches no gradient
        out = RC.forward(im1, im2, md)
        ring = ~RC.inner(12, 15, md)
        assert (out[:, 0][:, ring] == 0).all() and (out[:, 0][:, ~ring] > 0).all()
        go_ring = go * ring[None, None]
        g1, g2, A = RC.backward(im1, im2, go_ring, md)
        assert np.abs(go_ring).max() > 0 and (g1 == 0).all() and (g2 == 0).all() and (A == 0).all()
        g1, g2, A = RC.backward(im1, im2, go, md)
        g1b, g2b, _ = RC.backward(im1, im2, go * ~ring[None, None], md)
        assert np.array_equal(g1, g1b) and np.array_equal(g2, g2b) and np.abs(g1).max() > 0
    # H < P or W < P: all zero
    for shape, md in (((1, 1, 6, 20), 3), ((2, 3, 20, 4), 2), ((1, 1, 2, 2), 1), ((1, 3, 1, 1), 1)):
        im1, im2, go = RC.image_pair(shape, 3)
        g1, g2, A = RC.backward(im1, im2, go, md)
        assert (RC.forward(im1, im2, md) == 0).all() and (g1 == 0).all() and (g2 == 0).all() and (A == 0).all()
        t = RC.compose(torch.from_numpy(im1), torch.from_numpy(im2), md)
        assert t.shape == (shape[0], 1) + shape[2:] and float(t.abs().max()) == 0
    # a flat im1 and a single interior pixel of im2 raised by delta (C = 1): with v = h(f(scale delta)) the output is
    # (K - 1) / K v at that pixel, v / K at every interior pixel within md of it, 0 elsewhere
    for md in (1, 2, 3):
        K = (2 * md + 1) ** 2
        H, W, y0, x0, delta, scale = 15, 17, md, 3 + md, 0.25, 8.0
        im1 = np.full((1, 1, H, W), 0.5, np.float32)
        im2 = im1.copy()
        im2[0, 0, y0, x0] += delta
        out = RC.forward(im1, im2, md, scale)[0, 0]
        v = RC.h(RC.f(scale * delta))
        want = np.zeros((H, W))
        yy, xx = np.mgrid[0:H, 0:W]
        near = (np.abs(yy - y0) <= md) & (np.abs(xx - x0) <= md) & RC.inner(H, W, md)
        want[near] = v / K
        want[y0, x0] = (K - 1) / K * v
        assert md <= y0 < H - md and near.sum() < K and near.sum() > 1      # the neighbourhood is cut by the ring (y0 = md)
        assert np.abs(out - want).max() <= 1e-15 and (out[~near] == 0).all()
        assert np.abs(RC.forward(im1, im2, md, scale, normalize=False)[0, 0] - K * want).max() <= 1e-13
    del rng


_ARITH_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "census_arith.h"
static float arg(unsigned bits) { float v; std::memcpy(&v, &bits, 4); return v; }
int main()
{
    char kind;
    unsigned a, b, c, d;
    while (std::scanf(" %c %x %x %x %x", &kind, &a, &b, &c, &d) == 5) {
        if (kind == 'g') std::printf("%a %a\n", census_grey3(arg(a), arg(b), arg(c), arg(d)), census_grey1(arg(a), arg(d)));
        else std::printf("%a %a %a %a %a\n", census_f(arg(a)), census_df(arg(a)), census_h(arg(a)), census_dh(arg(a)), census_tap(arg(a), arg(b)));
    }
    return 0;
}
"""


def test_arithmetic_header_under_the_undefined_behaviour_sanitizer(tmp_path):
    """csrc/census_arith.h in a stand-alone program (its own main), built with the undefined-behaviour sanitizer without recovery
    and without contraction: grey bit for bit against the numpy float32 restatement, f, f', h, h' and a tap within their per-tap
    bounds against float64."""
    src, exe = tmp_path / "arith.cpp", tmp_path / "arith"
    src.write_text(_ARITH_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                        "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    f32 = np.float32
    tiny = f32(1e-30)
    xs = [f32(v) for v in (0.0, -0.0, tiny, -tiny, 1e-40, -1e-40, 0.9, -0.9, 255.0, -255.0, 2.0 ** 59, -2.0 ** 59, 0.18257, 3.0, -0.01)]
    rng = np.random.default_rng(9)
    triples = [(f32(0), f32(0), f32(0)), (f32(1), f32(1), f32(1)), (f32(0.5), f32(0.25), f32(0.125)), (f32(1e-30), f32(1), f32(1e30))]
    triples += [tuple(rng.random(3).astype(f32)) for _ in range(40)]
    scales = [f32(255.0), f32(1.0), f32(8.0)]
    bits = lambda v: int(np.asarray(v, f32).view(np.uint32))     # noqa: E731
    lines, cases = [], []
    for x in xs:
        for y in xs[:9]:
            lines.append("x %08x %08x 0 0" % (bits(x), bits(y)))
            cases.append(("x", x, y))
    for (r_, g_, b_) in triples:
        for s in scales:
            lines.append("g %08x %08x %08x %08x" % (bits(r_), bits(g_), bits(b_), bits(s)))
            cases.append(("g", r_, g_, b_, s))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    for case, line in zip(cases, out):
        got = [float.fromhex(t) for t in line.split()]
        if case[0] == "g":
            _, r_, g_, b_, s = case
            with np.errstate(over="ignore"):
                want3 = RC.grey(np.array([r_, g_, b_], f32).reshape(1, 3, 1, 1), s)[0, 0, 0]
                want1 = RC.grey(np.array([r_], f32).reshape(1, 1, 1, 1), s)[0, 0, 0]
            assert f32(got[0]).view(np.uint32) == want3.view(np.uint32) and f32(got[1]).view(np.uint32) == want1.view(np.uint32), case
            continue
        _, x, y = case
        x64, y64 = float(x), float(y)
        fx, dfx, hx, dhx, tap = got
        # f: 5 u of a value below 1; f' <= 1.12: 13 u; h (of d = x) <= 1: 6 u; h' <= 2.06: 8 u relative; a tap: the header's 32 u
        assert abs(fx - RC.f(x64)) <= 5 * U and abs(fx) <= 1.0
        assert abs(dfx - RC.df(x64)) <= 13 * U * 1.12
        assert abs(hx - RC.h(x64)) <= 6 * U and 0.0 <= hx <= 1.0
        assert abs(dhx - RC.dh(x64)) <= 8 * U * 2.06
        assert abs(tap - RC.h(RC.f(x64) - RC.f(y64))) <= 32 * U
        if x64 == 0.0:
            assert fx == 0.0 and hx == 0.0 and dhx == 0.0 and dfx == pytest.approx(0.81 ** -0.5, rel=1e-6)
        if x64 == y64:
            assert tap == 0.0


def test_kernels_use_no_scratch_and_their_lds_is_the_headers_formula(tmp_path):
    """0 bytes of scratch for every instantiation -- three forward kernels (max_distance 1, 2, 3) and nine backward kernels (both
    gradients, the first, the second) -- and each kernel's LDS is exactly FN2C_LDS_BYTES: 2 (forward) or 3 (backward) planes of
    (16 + 2 md) x (64 + 2 md + FN2C_PAD) floats; device code only, the library's own flags."""
    import build
    src = os.path.join(PKG, "csrc", "census.hip")
    r = subprocess.run([build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "census.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S*census_\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", r.stderr, flags=re.S)
    names = [k for k, _, _ in kernels]
    assert sum("census_fwd" in k for k in names) == 3 and sum("census_bwd" in k for k in names) == 9 and len(names) == 12, names
    m = RC.header_macros()
    assert (m["FN2C_TILE_H"], m["FN2C_TILE_W"]) == (16, 64)
    seen = set()
    for name, body, lds in kernels:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
        assert scratch == 0, f"{name} spills {scratch} bytes per lane"
        kind, md = re.search(r"census_(fwd|bwd)ILi(\d)E", name).groups()
        md = int(md)
        planes = 2 if kind == "fwd" else 3
        want = planes * 4 * (16 + 2 * md) * (64 + 2 * md + m["FN2C_PAD"])
        assert want == RC.lds_bytes(planes, md) and int(lds) == want, f"{name} uses {lds} bytes of LDS, expected {want}"
        seen.add((kind, md))
    assert seen == {(k, d) for k in ("fwd", "bwd") for d in (1, 2, 3)}
    assert RC.lds_bytes(2, 3) == 12496 and RC.lds_bytes(3, 3) == 18744 <= 64 * 1024


# ------------------------------------------------------------------ the image families
_FAMILY_SHAPES = ((1, 1, 17, 67), (2, 3, 33, 130))
_FAMILY_CONFIGS = ((1, True), (3, False), (3, True))


def _emulated_ratios(shape, family, scale, md, normalize, mutate=None):
    """Largest error / bound of the float32 emulation of the header's operation list: (forward, grad_im1, grad_im2); everything
    finite, and exactly 0 where A = 0 and on the ring."""
    im1, im2, _ = RC.image_family(family, shape, 40 + shape[2])
    go = RC.grad_out(shape, 41 + shape[2])
    out = RC.forward(im1, im2, md, scale, normalize)
    g1, g2, A = RC.backward(im1, im2, go, md, scale, normalize)
    assert np.isfinite(out).all() and np.isfinite(g1).all() and np.isfinite(g2).all() and np.isfinite(A).all()
    o, e1, e2 = RC.emulate(im1, im2, go, md, scale, normalize, mutate)
    assert np.isfinite(o).all() and np.isfinite(e1).all() and np.isfinite(e2).all()
    ring = ~RC.inner(shape[2], shape[3], md)
    assert (o[:, 0][:, ring] == 0).all() and (e1[A == 0] == 0).all() and (e2[A == 0] == 0).all()
    gb = RC.backward_bound(A)
    pos = gb > 0
    return (float(np.abs(o - out).max() / RC.forward_bound(md, normalize)), float((np.abs(e1 - g1)[pos] / gb[pos]).max()),
            float((np.abs(e2 - g2)[pos] / gb[pos]).max()))


def test_image_families_keep_their_conditions():
    """Every family asserts in ``image_family`` what it is for; ``noise`` is the pair the other tests use; a family made benign
    is refused."""
    for shape in _FAMILY_SHAPES:
        for name in RC.FAMILIES:
            im1, im2, scale = RC.image_family(name, shape, 9)
            assert im1.shape == im2.shape == shape and scale == (1.0 if name == "graded" else 255.0)
        a, b, _ = RC.image_pair(shape, 9)
        im1, im2, _ = RC.image_family("noise", shape, 9)
        assert np.array_equal(a, im1) and np.array_equal(b, im2)
    assert {f for f, _ in RC.FAMILY_SCALES} == set(RC.FAMILIES)
    assert {s for f, s in RC.FAMILY_SCALES if f == "noise"} == {255.0, -255.0, 1.0, 2.0 ** -30}
    assert {s for f, s in RC.FAMILY_SCALES if f == "seams"} == {255.0, 1.0}
    # the conditions bite: each family's check on another family's images
    shape = _FAMILY_SHAPES[1]
    noise1, noise2, _ = RC.image_pair(shape, 9)
    for md in (3,):
        x1 = RC._taps(RC.grey(noise1, 255.0), md)
        assert (np.abs(x1) < 1.75).mean() < 0.5                                     # knee's
        d = RC.f(x1) - RC.f(RC._taps(RC.grey(noise2, 255.0), md))
        assert np.median(np.abs(d)) < 1.5                                           # opposed's
        assert RC.forward(noise1, noise2, md).max() > 1e-5                          # flat's
        assert np.abs(RC.grey(noise1, 1.0)).max() < 2.0 ** 57                       # graded's


def test_emulation_stays_inside_the_bounds_on_every_family():
    """The float32 emulation of the header's operation list stays inside the header's bounds, in full, on every family and scale;
    the worst error / bound per family is printed."""
    for family, scale in RC.FAMILY_SCALES:
        worst = np.zeros(3)
        for shape in _FAMILY_SHAPES:
            for md, normalize in _FAMILY_CONFIGS:
                worst = np.maximum(worst, _emulated_ratios(shape, family, scale, md, normalize))
        print(f"emulation, {family} at scale {scale:g}: forward {worst[0]:.4f}, grad_im1 {worst[1]:.4f}, grad_im2 {worst[2]:.4f}")
        assert worst.max() <= 1.0, (family, scale, worst)


@pytest.mark.parametrize("mutate,family,scale", [("abs_scale", "noise", -255.0), ("clamped_grey", "graded", 1.0), ("clamped_grey", "seams", 1.0)])
def test_a_planted_mistake_passes_the_original_family_and_fails_a_new_one(mutate, family, scale):
    """Teeth: a gradient scaled by |scale| and a grey intensity clamped to [0, 255] stay inside a quarter of the bounds on the
    original pair at scale 255 -- and leave the bounds on the negative scale, the graded magnitudes and the +-1 checkerboard."""
    shape, md, normalize = _FAMILY_SHAPES[1], 3, True
    assert max(_emulated_ratios(shape, "noise", 255.0, md, normalize, mutate)) <= 0.25
    bad, clean = _emulated_ratios(shape, family, scale, md, normalize, mutate), _emulated_ratios(shape, family, scale, md, normalize)
    print(f"{mutate} on {family} at scale {scale:g}: error / bound {max(bad):.3g}, without the mistake {max(clean):.4f}")
    assert max(bad) > 1 and max(clean) <= 1
