"""CPU-side checks of the staging library libflownet2_hip_ssim.so (include/staging/flownet2_hip_ssim.h; SSIMLoss).

The float64 reference (tests/ssim_ref.py: the header's gather form, and under reflect the adjoint of the padding) against autograd of
the PyTorch composition; the input families keep off the clamp's ends; the staging record -- the descriptor, exports == header ==
fn2_capi, ABI version 0, nothing linked, the prefix its own, the module linking exactly its library -- written so that it names
its own entry and never the stage's size; the header compiles as C99 alone and after each released and preview header; every
rejection in front of a launch (host pointers, no GPU); STATUS_SSIM's texts; the operator listings; SSIMLoss under fake tensors
without a graph break.
"""
import ctypes
import math
import os
import re
import subprocess
import sys
import sysconfig

import pytest
import torch

from conftest import PKG, ROOT

import build
import fn2_capi
import ssim_ref as R
from test_corr_sample_host import RELEASED_HEADERS
from test_libraries_host import _declared, _exported, _needed

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
NAMES = ["fn2i_abi_version", "fn2i_ssim_backward", "fn2i_ssim_forward"]
PREVIEW_HEADERS = ["preview/flownet2_hip_sample.h", "preview/flownet2_hip_pyramid.h"]
META = torch.device("meta")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("border", ["zero", "reflect"])
@pytest.mark.parametrize("md", [1, 2, 3])
def test_reference_gradient_against_autograd_of_the_composition(md, border):
    """Values and both gradients of the header's form, in float64, against the raw-moment composition under autograd."""
    x, y, go = R.inputs((2, 3, 19, 37), "noise", seed=md)
    ref = R.reference(x, y, go, md, R.C1, R.C2, border)
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    out = R.compose(a, b, md, R.C1, R.C2, border)
    w1, w2 = torch.autograd.grad(out, (a, b), go)
    assert float((out.detach() - ref["out"]).abs().max()) <= 1e-13
    assert ref["margin"] > 4           # off the clamp's ends: the clamp passes everywhere
    for got, want in ((ref["g1"], w1), (ref["g2"], w2)):
        assert float(want.abs().max()) > 0.1
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    if border == "zero":
        ring = R.valid_mask(x.shape, md, border) == 0
        assert bool((ref["out"][ring.expand_as(x)] == 0).all()) and bool((ref["bound"][ring.expand_as(x)] == 0).all())


@pytest.mark.parametrize("family", ["noise", "smooth", "bytes"])
def test_families_keep_off_the_clamp(family):
    """0 < (1 - S) / 2 < 1 with a margin of at least four forward bounds, for md 1 - 3 and both borders: which side of the clamp an
    element is on is never a matter of rounding in the GPU tests."""
    c1, c2 = R.constants(family)
    for md in (1, 2, 3):
        for border in ("zero", "reflect"):
            x, y, _ = R.inputs((2, 3, 2 * R.TILE_H + md, 2 * R.TILE_W + 2 * md + 1), family)
            ref = R.reference(x, y, None, md, c1, c2, border)
            assert 4 < ref["margin"] < float("inf"), (md, border, ref["margin"])
            inner = R.valid_mask(x.shape, md, border).expand_as(x) > 0
            assert float(ref["out"][inner].min()) > 0 and float(ref["out"][inner].max()) < 1


def test_the_float32_composition_is_no_better_than_the_bound_promises():
    """On smooth images the raw moments cancel against c2: the float32 composition's error exceeds the header's bound, which a
    kernel that inherited that form could not meet."""
    x, y, _ = R.inputs((1, 1, 33, 65), "smooth")
    ref = R.reference(x, y, None, 3, R.C1, R.C2, "reflect")
    err = (R.compose(x.float(), y.float(), 3, R.C1, R.C2, "reflect").double() - ref["out"]).abs()
    assert float((err / ref["bound"]).max()) > 1.0


# ------------------------------------------------------------------ the staging record
def test_staging_descriptor():
    assert "ssim" in build.STAGING
    desc = build.STAGING["ssim"]
    assert desc.srcs == ["capi_ssim.hip", "ssim.hip"] and desc.modules == ["ssim_cuda"]
    assert desc.link == "flownet2_hip_ssim" and desc.vmap == "exports_ssim.map" and desc.header == "staging/flownet2_hip_ssim.h"
    assert type(desc) is type(build.LIBRARIES[""])
    assert build.ALL_TABLES == build.TABLES + (build.STAGING,) and build._described("ssim") is desc
    assert "ssim_cuda" not in build.MODULES and len(build.MODULES) == 10
    # whatever else the stage holds, it shares no name and no module with the closed tables
    for table in build.TABLES:
        assert not set(table) & set(build.STAGING)
        assert not {m for lib in table.values() for m in lib.modules} & {m for lib in build.STAGING.values() for m in lib.modules}
    assert os.path.isfile(os.path.join(ROOT, "include", desc.header)) and os.path.isfile(os.path.join(PKG, "csrc", desc.vmap))


def test_library_exports_what_its_header_declares():
    desc = build.STAGING["ssim"]
    path = fn2_capi.SSIM_LIB_PATH
    assert os.path.samefile(path, os.path.join(PKG, "lib", "lib%s.so" % desc.link))
    assert fn2_capi.ssim_lib().fn2i_abi_version() == 0 == R.M["FN2I_ABI_VERSION"]
    assert _exported(path) == _declared(desc.header, "fn2i_") == sorted(fn2_capi.SSIM_EXPORTS) == NAMES
    assert _needed(path) == []
    # no other library, the debug twin included, exports an fn2i_ name
    for table in build.TABLES:
        for name in table:
            stem = name.upper() + "_" if name else ""
            assert not any(n.startswith("fn2i_") for n in getattr(fn2_capi, stem + "EXPORTS")), name
            assert not any(n.startswith("fn2i_") for n in _exported(getattr(fn2_capi, stem + "LIB_PATH"))), name
    assert not any(n.startswith("fn2i_") for n in fn2_capi.DEBUG_EXPORTS)


def test_module_links_exactly_its_library():
    assert _needed(os.path.join(PKG, "ssim_cuda" + sysconfig.get_config_var("EXT_SUFFIX"))) == ["libflownet2_hip_ssim.so"]
    text = open(os.path.join(PKG, "csrc", "binding", "ssim_cuda.cpp")).read()
    assert "STATUS_SSIM" in text and "fn2_strerror(" not in text
    for table in build.TABLES:
        for lib in table.values():
            for module in lib.modules:
                assert "STATUS_SSIM" not in open(os.path.join(PKG, "csrc", "binding", module + ".cpp")).read(), module


def test_kernels_use_no_memset_and_no_inline_assembly():
    for src in build.STAGING["ssim"].srcs + ["ssim.h"]:
        text = open(os.path.join(PKG, "csrc", src)).read()
        assert "hipMemset" not in text and not re.search(r"\basm\b|__asm", text), src


def test_header_compiles_alone_and_after_the_others(tmp_path):
    orders = [[], RELEASED_HEADERS, RELEASED_HEADERS + PREVIEW_HEADERS] + [[h] for h in RELEASED_HEADERS + PREVIEW_HEADERS]
    for i, incs in enumerate(orders):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in list(incs) + ["staging/flownet2_hip_ssim.h"]) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2I_MAX_DISTANCE + FN2I_TILE_H + FN2I_BORDER_REFLECT + FN2I_ABI_VERSION];\n"
                       "int lds[FN2I_LDS_FWD(3) + FN2I_LDS_BWD(3)];\n"
                       "double bound = FN2I_BOUND_SLACK * (FN2I_BOUND_MEAN + FN2I_BOUND_MOMENT + FN2I_BOUND_TAP);\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (incs, r.stderr)


def test_header_macros():
    assert (R.M["FN2I_TILE_H"], R.M["FN2I_TILE_W"], R.M["FN2I_HALO_X"], R.M["FN2I_MAX_DISTANCE"]) == (16, 64, 4, 3)
    assert (R.M["FN2I_BORDER_ZERO"], R.M["FN2I_BORDER_REFLECT"]) == (0, 1) == (fn2_capi.FN2I_BORDER["zero"], fn2_capi.FN2I_BORDER["reflect"])
    assert R.M["FN2I_MAP_PITCH"] >= R.M["FN2I_TILE_W"] + 2 * R.M["FN2I_MAX_DISTANCE"]
    assert R.M["FN2I_BOUND_SLACK"] == 1 + 2.0 ** -8


# ------------------------------------------------------------------ rejections
def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.ssim_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    c1, c2 = 1e-4, 9e-4

    def fwd(a, b, N, C, H, W, md=1, c1=c1, c2=c2, border=0, out=p):
        return lib.fn2i_ssim_forward(a, b, out, N, C, H, W, md, c1, c2, border, null)

    def bwd(a, b, N, C, H, W, md=1, c1=c1, c2=c2, border=0, out=p):
        return lib.fn2i_ssim_backward(a, b, p, out, out, N, C, H, W, md, c1, c2, border, null)

    for call in (fwd, bwd):
        # 1. sizes, whatever else is wrong
        for N, C, H, W in ((-1, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, -3)):
            assert call(null, null, N, C, H, W, md=0) == EINVAL, (N, C, H, W)
        # 2. limits
        assert call(null, null, 1, 1, 65536, 32768) == EUNSUPPORTED
        assert call(null, null, 1 << 16, 1 << 15, 8, 8) == EUNSUPPORTED
        assert call(null, null, 1 << 15, 1 << 10, 1 << 12, 1 << 12) == EUNSUPPORTED
        assert call(null, null, 0, 1, 65536, 32768) == EUNSUPPORTED                 # limits before the empty batch
        # 3. the parameters, before the empty batch and the pointers
        for md in (0, 4, -1):
            assert call(p, p, 1, 1, 8, 8, md=md) == EINVAL, md
            assert call(p, p, 0, 1, 8, 8, md=md) == EINVAL, md
        for bad in (0.0, -1e-4, math.inf, math.nan, -math.inf):
            assert call(p, p, 1, 1, 8, 8, c1=bad) == EINVAL, bad
            assert call(p, p, 1, 1, 8, 8, c2=bad) == EINVAL, bad
        for border in (-1, 2):
            assert call(p, p, 1, 1, 8, 8, border=border) == EINVAL, border
        for md, H, W in ((1, 1, 8), (2, 8, 2), (3, 3, 3)):
            assert call(p, p, 1, 1, H, W, md=md, border=1) == EINVAL, (md, H, W)   # reflect needs H > md and W > md
            assert call(p, p, 0, 1, H, W, md=md, border=0) == OK, (md, H, W)       # zero mode takes any size
        # 4. the empty batch: nothing to do, whatever the pointers
        assert call(null, null, 0, 3, 8, 8) == OK
        assert call(mis, null, 0, 3, 8, 8, border=1) == OK
        # 5. NULL, also next to a misaligned pointer: NULL is reported first
        assert call(null, p, 1, 1, 8, 8) == EINVAL
        assert call(mis, null, 1, 1, 8, 8) == EINVAL
        assert call(p, p, 1, 1, 8, 8, out=null) == EINVAL            # the forward's output; both gradients of the backward
        # 6. alignment to 4 bytes
        assert call(mis, p, 1, 1, 8, 8) == EALIGN
        assert call(p, mis, 1, 1, 8, 8) == EALIGN
        assert call(p, p, 1, 1, 8, 8, out=mis) == EALIGN
    assert lib.fn2i_ssim_backward(p, p, null, p, p, 1, 1, 8, 8, 1, c1, c2, 0, null) == EINVAL
    assert lib.fn2i_ssim_backward(p, p, mis, p, p, 1, 1, 8, 8, 1, c1, c2, 0, null) == EALIGN
    assert lib.fn2i_ssim_backward(p, p, p, null, mis, 1, 1, 8, 8, 1, c1, c2, 0, null) == EALIGN   # one gradient alone may be NULL


STATUS_PROGRAM = """
#include <cstdio>
#include "binding_status.h"
int main()
{
    const int codes[] = {-1, -2, -3, -4, 7, -9};
    for (int rc : codes) std::puts(fn2b::status_message(fn2b::STATUS_SSIM, "op", rc).c_str());
    return 0;
}
"""


def test_status_text(tmp_path):
    src, exe = tmp_path / "status.cpp", tmp_path / "status"
    src.write_text(STATUS_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc", "binding"), "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines == [
        "op: HIP call failed: flownet2_hip_ssim: invalid shape or parameter (max_distance 1 .. 3, c1 and c2 finite and > 0, border reflect needs "
        "H and W above max_distance) (code -1)",
        "op: HIP call failed: flownet2_hip_ssim: unknown error (code -2)",
        "op: HIP call failed: flownet2_hip_ssim: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_ssim: unsupported size (a plane of 2^31 elements or more, or too many planes) (code -4)",
        "op: HIP call failed: flownet2_hip_ssim: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_ssim: unknown error (code -9)"]


def test_binding_refuses_with_the_argument_and_the_remedy():
    import ssim_cuda
    from networks.ssim_package import SSIM, SSIMLoss, ssim_distance
    a = torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="im1 must be a GPU .HIP. tensor; this extension has no CPU implementation"):
        ssim_distance(a, a)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(RuntimeError, match=r"im1 must be float32, got .*: convert it with \.float\(\)"):
            ssim_distance(a.to(dt), a.to(dt))
        with pytest.raises(RuntimeError, match=r"im2 must be float32, got .*: convert it with \.float\(\)"):
            ssim_distance(a, a.to(dt))
    with pytest.raises(RuntimeError, match="max_distance 4 is not 1, 2 or 3"):
        ssim_distance(a, a, md=4)
    with pytest.raises(RuntimeError, match="c1 0 is not a finite float above 0"):
        ssim_distance(a, a, c1=0.0)
    with pytest.raises(RuntimeError, match="c2 .* is not a finite float above 0"):
        ssim_distance(a, a, c2=float("nan"))
    with pytest.raises(RuntimeError, match=r"must have the shape of im1"):
        ssim_distance(a, a[:, :1])
    with pytest.raises(RuntimeError, match="border reflect needs H and W above max_distance 3, got 3 x 8: use border zero or a smaller max_distance"):
        ssim_distance(a[:, :, :3], a[:, :, :3], md=3, border="reflect")
    with pytest.raises(RuntimeError, match="border code 5 is not 0 .zero. or 1 .reflect."):
        ssim_cuda.forward_alloc(a, a, 1, 1e-4, 9e-4, 5)
    with pytest.raises(RuntimeError, match="neither gradient is wanted"):
        ssim_cuda.backward_alloc(a, a, a, 1, 1e-4, 9e-4, 0, False, False)
    with pytest.raises(ValueError, match="border 'wrap' is not 'zero' or 'reflect'"):
        ssim_distance(a, a, border="wrap")
    with pytest.raises(ValueError, match="md 0 is not 1, 2 or 3"):
        SSIM(md=0)
    assert "md=2" in repr(SSIMLoss(md=2, border="reflect")) and "border='reflect'" in repr(SSIMLoss(md=2, border="reflect"))


# ------------------------------------------------------------------ the operators
_LISTINGS = """
import importlib, sys
import torch, fn2_ops
for m in ("networks.census_package.census", "networks.correlation_package.corr_block", "networks.correlation_package.corr_pyramid"):
    importlib.import_module(m)
before = (fn2_ops.names(), fn2_ops.names(preview=True), fn2_ops.names(incubating=True))
assert all(before) and fn2_ops.names(staging=True) == []
ext = {m for m in sys.modules if m.endswith("_cuda")}
importlib.import_module("networks.ssim_package.ssim")
assert (fn2_ops.names(), fn2_ops.names(preview=True), fn2_ops.names(incubating=True)) == before
assert fn2_ops.names(staging=True) == ["fn2::ssim", "fn2::ssim_backward"], fn2_ops.names(staging=True)
assert not set(fn2_ops.names(staging=True)) & set(before[0] + before[1] + before[2])
assert {m for m in sys.modules if m.endswith("_cuda")} - ext == {"ssim_cuda"}
print("listed")
"""


def test_staging_operators_are_in_no_other_listing():
    code = "import sys; sys.path[:0] = %r\n" % [PKG, ROOT] + _LISTINGS
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert res.returncode == 0 and "listed" in res.stdout, res.stderr[-2000:]


def test_nothing_existing_imports_the_new_package():
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py") and "ssim_package" not in d:
                assert "ssim_package" not in open(os.path.join(d, f)).read(), os.path.join(d, f)


@pytest.mark.parametrize("border", ["zero", "reflect"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_ssim_loss_traces_without_a_graph_break(border, masked):
    from networks.ssim_package import SSIMLoss
    loss = SSIMLoss(md=2, border=border)
    a = torch.empty(2, 3, 9, 11, device=META, requires_grad=True)
    b = torch.empty(2, 3, 9, 11, device=META, requires_grad=True)
    mask = torch.empty(2, 1, 9, 11, device=META) if masked else None
    torch._dynamo.reset()
    out = torch.compile(loss, backend="aot_eager", fullgraph=True)(a, b, mask)
    assert out.device.type == "meta" and out.shape == () and out.requires_grad
    g1, g2 = torch.autograd.grad(out, (a, b))
    assert g1.shape == a.shape and g2.shape == b.shape and g1.dtype == torch.float32
    torch._dynamo.reset()
    rep = torch._dynamo.explain(loss)(a, b, mask)
    assert rep.graph_break_count == 0 and rep.graph_count == 1, rep.break_reasons


def test_operators_refuse_at_trace_time_and_not_twice():
    import networks.ssim_package.ssim as Mod
    a = torch.empty(1, 1, 8, 8, device=META)
    assert torch.ops.fn2.ssim(a, a, 1, 1e-4, 9e-4, 0).shape == a.shape
    g1, g2 = torch.ops.fn2.ssim_backward(a, a, a, 1, 1e-4, 9e-4, 0, True, False)
    assert g1.shape == a.shape and g2.numel() == 0
    with pytest.raises(RuntimeError, match="fn2::ssim: max_distance 4 is not 1, 2 or 3"):
        torch.ops.fn2.ssim(a, a, 4, 1e-4, 9e-4, 0)
    with pytest.raises(RuntimeError, match=r"fn2::ssim: im1 must be float32, got torch.float16: convert it with \.float\(\)"):
        torch.ops.fn2.ssim(a.half(), a.half(), 1, 1e-4, 9e-4, 0)
    with pytest.raises(RuntimeError, match="fn2::ssim: border reflect needs H and W above max_distance"):
        torch.ops.fn2.ssim(a[:, :, :2], a[:, :, :2], 2, 1e-4, 9e-4, 1)
    # the constants are judged as the float32 numbers the kernel gets, at trace time as at the binding's door
    import ssim_cuda
    cpu = torch.zeros(1, 1, 8, 8)
    for bad in (1e-60, 1e60, 0.0, -1.0, float("nan")):
        for kw in ({"c1": bad, "c2": 9e-4}, {"c1": 1e-4, "c2": bad}):
            name = "c1" if kw["c1"] == bad or bad != bad and kw["c2"] == 9e-4 else "c2"
            with pytest.raises(RuntimeError, match=f"fn2::ssim: {name} .* is not a finite float above 0"):
                torch.ops.fn2.ssim(a, a, 1, kw["c1"], kw["c2"], 0)
            with pytest.raises(RuntimeError, match=f"ssim_cuda.forward_alloc: {name} .* is not a finite float above 0"):
                ssim_cuda.forward_alloc(cpu, cpu, 1, kw["c1"], kw["c2"], 0)
    assert torch.ops.fn2.ssim(a, a, 1, 1e-44, 3e38, 0).shape == a.shape      # a denormal and a large float32 are numbers
    for empty in ((1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0)):
        e = torch.empty(empty, device=META)
        with pytest.raises(RuntimeError, match="fn2::ssim: the images .* have an empty channel, row or column dimension"):
            torch.ops.fn2.ssim(e, e, 1, 1e-4, 9e-4, 0)
        with pytest.raises(RuntimeError, match="ssim_cuda.forward_alloc: the images .* have an empty channel, row or column dimension"):
            ssim_cuda.forward_alloc(torch.empty(empty), torch.empty(empty), 1, 1e-4, 9e-4, 0)
    assert torch.ops.fn2.ssim(a[:0], a[:0], 1, 1e-4, 9e-4, 1).shape == (0, 1, 8, 8)   # an empty batch is not an empty image
    b = a.clone().requires_grad_(True)
    g, _ = torch.ops.fn2.ssim_backward(b, a, a, 1, 1e-4, 9e-4, 0, True, False)
    with pytest.raises(RuntimeError, match="fn2::ssim_backward: the backward of this layer is a HIP kernel and not differentiable a second time"):
        g.sum().backward()
    assert Mod.BORDERS == {"zero": 0, "reflect": 1}
