"""CPU-side checks of the staging library libflownet2_hip_sample1d.so (include/staging/flownet2_hip_sample1d.h; CorrSample1d /
CorrBlock1D).

The float64 reference (tests/corr_sample1d_ref.py) against RAFT-Stereo's composition and its autograd, the channel and level order,
the y channel's irrelevance; the staging record -- the descriptor, exports == header == fn2_capi, ABI version 0, nothing linked, the
prefix its own, the module linking exactly its library -- written so that it names its own entry and never the stage's size; the
header compiles as C99 alone and after each released, preview and staging header; every rejection in front of a launch (host
pointers, no GPU); STATUS_SAMPLE1D's texts; the binding's refusals; the operator listings; CorrBlock1D under fake tensors without a
graph break; the float32 composition's own error, which the GPU test's acceptance rule leans on.
"""
import ctypes
import os
import re
import subprocess
import sys
import sysconfig

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import build
import corr_sample1d_ref as R
import fn2_capi
from test_corr_sample_host import RELEASED_HEADERS
from test_libraries_host import _declared, _exported, _needed

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
NAMES = ["fn2h_abi_version", "fn2h_corr_sample1d_backward", "fn2h_corr_sample1d_forward"]
OTHER_HEADERS = ["preview/flownet2_hip_sample.h", "preview/flownet2_hip_pyramid.h", "staging/flownet2_hip_ssim.h"]
META = torch.device("meta")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("geo", [(2, 9, 21, 4, 2), (3, 7, 8, 2, 1), (1, 11, 19, 3, 4), (2, 4, 4, 1, 0)], ids=lambda g: "%dx%d-W2_%d-L%d-r%d" % g)
def test_reference_against_raft_stereos_composition(geo):
    """Values to 1e-12 relative and the gradients of the levels against autograd of the composition, in float64, level widths >= 2;
    coordinates at non-negative positions or below -2^(L-1), where fl32(c - floor(c)) is exact at every level (the header)."""
    H, W, W2, L, r = geo
    B = 2
    rng = np.random.default_rng(H + r)
    widths = R.pyramid_widths(W2, L)
    assert widths[-1] >= 2
    pyr = [torch.from_numpy(rng.standard_normal((B * H * W, 1, 1, w))).requires_grad_(True) for w in widths]
    c = rng.uniform(-r - 2, W2 + r + 2, (B, 1, H, W))
    c = np.where(c < 0, c - 2.0 ** (L - 1), c).astype(np.float32)
    go = rng.standard_normal((B, L * (2 * r + 1), H, W))
    want = R.compose_lookup(pyr, torch.from_numpy(c).double(), r)
    wgrads = torch.autograd.grad(want, pyr, torch.from_numpy(go))
    got, S = R.forward([t.detach().numpy() for t in pyr], c, r)
    scale = float(want.detach().abs().max())
    assert got.shape == tuple(want.shape) and scale > 0.1 and np.abs(got - want.detach().numpy()).max() <= 1e-12 * scale
    assert (S >= np.abs(got) - 1e-15).all()
    for (g, Sg, n), w in zip(R.backward(widths, c, go, r), wgrads):
        w = w.numpy().reshape(g.shape)
        assert float(np.abs(w).max()) > 0.1 and np.abs(g - w).max() <= 1e-12 * float(np.abs(w).max())
        assert (g[n == 0] == 0).all() and (Sg[n == 0] == 0).all() and 1 <= int(n.max()) <= 2


def test_channel_and_level_order():
    """A one-hot level: level 1's only non-zero cell of every slice is cell 3; the integer coordinate 6 / 2 = 3 puts it in the
    window's centre, channel D + r; the coordinate 4 sees it at offset i - r = +1; 7 / 2 = 3.5 splits it between offsets 0 and -1."""
    r, L, H, W = 2, 3, 1, 3
    D = 2 * r + 1
    levels = [np.zeros((H * W, 8 >> l)) for l in range(L)]
    levels[1][:, 3] = 1.0
    co = np.array([[[[6.0, 4.0, 7.0]]]], dtype=np.float32)
    out, _ = R.forward(levels, co, r)
    assert out.shape == (1, L * D, H, W)
    assert out[0, :, 0, 0].nonzero()[0].tolist() == [D + r] and out[0, D + r, 0, 0] == 1.0
    assert out[0, :, 0, 1].nonzero()[0].tolist() == [D + r + 1]
    assert out[0, :, 0, 2].nonzero()[0].tolist() == [D + r - 1, D + r] and out[0, D + r, 0, 2] == 0.5
    # the composition agrees on that order
    comp = R.compose_lookup([torch.from_numpy(t).reshape(H * W, 1, 1, -1) for t in levels], torch.from_numpy(co).double(), r)
    assert np.abs(comp.numpy() - out).max() <= 1e-15
    # the backward sends channel D + r of pixel 0 back to that cell, and nothing anywhere else
    go = np.zeros_like(out)
    go[0, D + r, 0, 0] = 1.0
    ref = R.backward([t.shape[1] for t in levels], co, go, r)
    assert ref[1][0][0, 3] == 1.0 and sum(float(np.abs(g).sum()) for g, _, _ in ref) == 1.0


def test_the_y_channel_has_no_influence():
    rng = np.random.default_rng(7)
    levels = [rng.standard_normal((2 * 3 * 5, w)) for w in (9, 4)]
    cx = R.coords("e", 2, 3, 5, 9, 2, seed=1).numpy()
    two = np.concatenate([cx, np.full_like(cx, np.nan)], axis=1)
    (a, Sa), (b, Sb) = R.forward(levels, cx, 2), R.forward(levels, two, 2)
    assert np.array_equal(a, b) and np.array_equal(Sa, Sb) and np.abs(a).max() > 0.1


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_coordinate_families(fam):
    """What each family promises (the GPU tests lean on it)."""
    B, H, W, W2, r = 2, 3, 37, 21, 4
    c = R.coords(fam, B, H, W, W2, r, seed=3).numpy()
    assert c.shape == (B, 1, H, W) and c.dtype == np.float32
    ok, v = R.has_taps(c), c[:, 0]
    if fam == "g":
        assert not ok.all() and ok.any() and np.isnan(v).any() and np.isinf(v).any() and (np.abs(v[np.isfinite(v)]) >= 2.0 ** 20).any()
    else:
        assert ok.all()
    if fam == "a":
        assert (v >= 0).all() and (v <= W2 - 0.5).all() and (v != np.floor(v)).mean() > 0.9
    if fam == "b":
        assert (v == np.floor(v)).all() and v.min() < 0 and v.max() >= W2
    if fam == "c":
        assert ((v > -1) & (v < 0)).any() and (v < -r).any() and (v > W2 - 1).any()
    if fam == "d":
        assert ((v < -r - 2) | (v > W2 + r + 1)).all() and (v < 0).any() and (v > 0).any()
        assert (R.forward([np.ones((B * H * W, W2))], c, r)[1] == 0).all()


def test_the_float32_compositions_own_error_is_not_zero():
    """The acceptance rule of DESIGN.md 4.16 in tests/test_gpu_corr_block1d.py, max(8 max|T_32 - T_64|, 2^-20 max|T_64|), is not
    vacuous at that test's shape: the float32 composition errs, in the output and in both feature gradients."""
    from test_gpu_corr_block1d import block_case, composed
    case = block_case()
    o64, o32 = composed(case, torch.float64), composed(case, torch.float32)
    for k in ("out", "fmap1.grad", "fmap2.grad"):
        err, scale = float((o32[k].double() - o64[k]).abs().max()), float(o64[k].abs().max())
        assert scale > 0.1 and 0 < err < 1e-4 * scale, (k, err, scale)


# ------------------------------------------------------------------ the staging record
def test_staging_descriptor():
    assert "sample1d" in build.STAGING
    desc = build.STAGING["sample1d"]
    assert desc.srcs == ["capi_sample1d.hip", "corr_sample1d.hip"] and desc.modules == ["corr_sample1d_cuda"]
    assert desc.link == "flownet2_hip_sample1d" and desc.vmap == "exports_sample1d.map" and desc.header == "staging/flownet2_hip_sample1d.h"
    assert type(desc) is type(build.LIBRARIES[""])
    assert build.ALL_TABLES == build.TABLES + (build.STAGING,) and build._described("sample1d") is desc
    assert "corr_sample1d_cuda" not in build.MODULES
    for table in build.TABLES:
        assert "sample1d" not in table and not any("corr_sample1d_cuda" in lib.modules for lib in table.values())
    assert os.path.isfile(os.path.join(ROOT, "include", desc.header)) and os.path.isfile(os.path.join(PKG, "csrc", desc.vmap))


def test_library_exports_what_its_header_declares():
    desc = build.STAGING["sample1d"]
    path = fn2_capi.SAMPLE1D_LIB_PATH
    assert os.path.samefile(path, os.path.join(PKG, "lib", "lib%s.so" % desc.link))
    assert fn2_capi.sample1d_lib().fn2h_abi_version() == 0 == R.header_macros()["FN2H_ABI_VERSION"]
    assert _exported(path) == _declared(desc.header, "fn2h_") == sorted(fn2_capi.SAMPLE1D_EXPORTS) == NAMES
    assert _needed(path) == []
    # no other library, the debug twin included, exports an fn2h_ name
    for table in build.ALL_TABLES:
        for name in table:
            if name == "sample1d":
                continue
            stem = name.upper() + "_" if name else ""
            assert not any(n.startswith("fn2h_") for n in getattr(fn2_capi, stem + "EXPORTS")), name
            assert not any(n.startswith("fn2h_") for n in _exported(getattr(fn2_capi, stem + "LIB_PATH"))), name
    assert not any(n.startswith("fn2h_") for n in fn2_capi.DEBUG_EXPORTS)


def test_module_links_exactly_its_library():
    assert _needed(os.path.join(PKG, "corr_sample1d_cuda" + sysconfig.get_config_var("EXT_SUFFIX"))) == ["libflownet2_hip_sample1d.so"]
    text = open(os.path.join(PKG, "csrc", "binding", "corr_sample1d_cuda.cpp")).read()
    assert "STATUS_SAMPLE1D" in text and "fn2_strerror(" not in text
    for table in build.ALL_TABLES:
        for lib in table.values():
            for module in lib.modules:
                if module != "corr_sample1d_cuda":
                    assert "STATUS_SAMPLE1D" not in open(os.path.join(PKG, "csrc", "binding", module + ".cpp")).read(), module


def test_kernels_use_no_memset_and_no_inline_assembly():
    """Neither in the library's own files nor through what they include: the project headers they pull in (csrc/fn2_common.h) do hold
    helpers written in inline assembly, and the sources must call none of them."""
    csrc = os.path.join(PKG, "csrc")
    own = build.STAGING["sample1d"].srcs + ["corr_sample1d.h"]
    texts = {src: re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(csrc, src)).read(), flags=re.S) for src in own}   # code, not comments
    for src, text in texts.items():
        assert "hipMemset" not in text and not re.search(r"\basm\b|__asm", text), src
    # the project headers reached from them, and the helpers there whose bodies hold assembly or a memset
    seen, todo = set(), [inc for t in texts.values() for inc in re.findall(r'#include "([^"]+)"', t)]
    tainted = set()
    while todo:
        path = os.path.normpath(os.path.join(csrc, todo.pop()))
        if path in seen or os.path.basename(path) in own or not path.startswith(csrc):
            continue        # (include/ holds declarations only: the C ABI headers)
        seen.add(path)
        text = open(path).read()
        todo += re.findall(r'#include "([^"]+)"', text)
        tainted |= set(re.findall(r"(\w+)\s*\([^()]*\)\s*\{[^{}]*(?:\basm\b|__asm|hipMemset)", text))
    assert os.path.join(csrc, "fn2_common.h") in seen and "store_out" in tainted, (seen, tainted)
    for src, text in texts.items():
        used = {name for name in tainted if re.search(r"\b%s\b" % name, text)}
        assert not used, f"{src} calls {sorted(used)}, written in inline assembly"


def test_kernels_use_no_scratch(tmp_path):
    """0 bytes of scratch for all 18 instantiations: the forward indexes the by-value parameter block with a
    wave-uniform level, which stays a scalar load; indexed per lane the block would be copied to scratch.  Device code only, the
    library's own flags, as tests/test_corr_lookup_host.py does it for its kernels."""
    M = R.header_macros()
    src = os.path.join(PKG, "csrc", "corr_sample1d.hip")
    r = subprocess.run([build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "corr_sample1d.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S*sample1d_(fwd|bwd)ILi(\d+)E\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", r.stderr, flags=re.S)
    assert sorted((k[1], int(k[2])) for k in kernels) == sorted((d, r_) for d in ("fwd", "bwd") for r_ in range(M["FN2H_MAX_RADIUS"] + 1))
    for name, direction, radius, body, lds in kernels:
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body).group(1))
        assert scratch == 0, f"{name} spills {scratch} bytes per lane"
        assert int(lds) <= 60 * 1024, f"{name} uses {lds} bytes of LDS"


def test_header_compiles_alone_and_after_the_others(tmp_path):
    every = RELEASED_HEADERS + OTHER_HEADERS
    assert all(os.path.isfile(os.path.join(ROOT, "include", h)) for h in every)
    for i, incs in enumerate([[], RELEASED_HEADERS, every] + [[h] for h in every]):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in list(incs) + ["staging/flownet2_hip_sample1d.h"]) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2H_MAX_LEVELS + FN2H_MAX_RADIUS - FN2H_BOUND_LOG2 + FN2H_ABI_VERSION];\n"
                       "int (*fwd)(const void *const *, const int *, int, const void *, long long, void *, int, int, int, int, void *)"
                       " = fn2h_corr_sample1d_forward;\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (incs, r.stderr)


def test_header_macros():
    M = R.header_macros()
    assert (M["FN2H_ABI_VERSION"], M["FN2H_MAX_LEVELS"], M["FN2H_MAX_RADIUS"], M["FN2H_BOUND_LOG2"]) == (0, 8, 8, -22)
    assert set(M) == {"FN2H_ABI_VERSION", "FN2H_MAX_LEVELS", "FN2H_MAX_RADIUS", "FN2H_BOUND_LOG2"}      # no tuning constant in the C ABI
    assert float(R.bound(1.0)) == 2.0 ** -22 + 4 * 2.0 ** -149 and (1 + 2.0 ** -24) ** 3 - 1 < 2.0 ** -22
    import networks.correlation_package.corr_block1d as Mod
    assert (Mod.MAX_LEVELS, Mod.MAX_RADIUS) == (M["FN2H_MAX_LEVELS"], M["FN2H_MAX_RADIUS"])


# ------------------------------------------------------------------ rejections
def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.sample1d_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 2)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*[x.value for x in v])

    def fwd(levels, W2, L, co, out, B, H, W, r, cbs=None):
        return lib.fn2h_corr_sample1d_forward(levels, W2, L, co, H * W if cbs is None else cbs, out, B, H, W, r, null)

    def bwd(levels, W2, L, co, go, B, H, W, r, cbs=None):
        return lib.fn2h_corr_sample1d_backward(W2, L, co, H * W if cbs is None else cbs, go, levels, B, H, W, r, null)

    w2, good = ints(8, 4), ptrs(p, p)
    for call in (fwd, bwd):
        # 1. parameters and sizes, whatever else is wrong
        for L in (0, -1, 9):
            assert call(None, None, L, null, null, 1, 8, 16, 4) == EINVAL, L
        for r in (-1, 9, 100):
            assert call(None, None, 2, null, null, 1, 8, 16, r) == EINVAL, r
        for B, H, W in ((-1, 8, 16), (1, 0, 16), (1, 8, 0), (1, -8, 16)):
            assert call(None, None, 2, null, null, B, H, W, 4, cbs=1 << 40) == EINVAL, (B, H, W)
        for bad in (ints(4, 0), ints(-4, 2)):
            assert call(None, bad, 2, null, null, 1, 8, 16, 4) == EINVAL
            assert call(None, bad, 2, null, null, 1, 65536, 65536, 4) == EINVAL       # sizes before the limits
        for cbs in (8 * 16 - 1, 0, -5):
            assert call(good, w2, 2, p, p, 1, 8, 16, 4, cbs=cbs) == EINVAL, cbs         # a batch stride below H W, also where B == 1
            assert call(good, w2, 2, p, p, 0, 8, 16, 4, cbs=cbs) == EINVAL, cbs         # ... and before the empty batch
        assert call(None, None, 2, null, null, 1, 65536, 32768, 4, cbs=5) == EINVAL     # ... and before the limits
        # 2. limits: B H W >= 2^31, more than 2^48 cells in a level
        assert call(None, None, 2, null, null, 1, 65536, 32768, 4) == EUNSUPPORTED
        assert call(None, None, 2, null, null, 4, 32768, 16384, 4) == EUNSUPPORTED
        assert call(None, ints(4, (1 << 28) + 1), 2, null, null, 1, 1024, 1024, 4) == EUNSUPPORTED     # 2^20 (2^28 + 1) cells
        assert call(None, ints(4, 1 << 28), 2, null, null, 1, 1024, 1024, 4) == EINVAL                 # 2^48 itself passes, to check 4
        assert call(None, w2, 2, null, null, 0, 65536, 32768, 4) == EUNSUPPORTED                       # limits before the empty batch
        # 3. the empty batch: nothing to do, whatever the pointers
        assert call(None, None, 2, null, null, 0, 8, 16, 4) == OK
        assert call(ptrs(mis, null), w2, 2, mis, null, 0, 8, 16, 4) == OK
        # 4. NULL arrays and pointers, also next to a misaligned one: NULL is reported first
        assert call(None, w2, 2, p, mis, 1, 8, 16, 4) == EINVAL
        assert call(good, None, 2, p, mis, 1, 8, 16, 4) == EINVAL
        assert call(good, w2, 2, null, mis, 1, 8, 16, 4) == EINVAL
        assert call(good, w2, 2, mis, null, 1, 8, 16, 4) == EINVAL
        assert call(ptrs(mis, null), w2, 2, p, p, 1, 8, 16, 4) == EINVAL
        assert call(ptrs(null, p), w2, 2, p, p, 1, 8, 16, 4) == EINVAL
        # 5. alignment to 4 bytes
        assert call(good, w2, 2, mis, p, 1, 8, 16, 4) == EALIGN
        assert call(good, w2, 2, p, mis, 1, 8, 16, 4) == EALIGN
        assert call(ptrs(p, mis), w2, 2, p, p, 1, 8, 16, 4) == EALIGN
        assert call(ptrs(mis, p), w2, 2, p, p, 1, 8, 16, 4, cbs=2 * 8 * 16) == EALIGN


STATUS_PROGRAM = """
#include <cstdio>
#include "binding_status.h"
int main()
{
    const int codes[] = {-1, -2, -3, -4, 7, -9};
    for (int rc : codes) std::puts(fn2b::status_message(fn2b::STATUS_SAMPLE1D, "op", rc).c_str());
    return 0;
}
"""


def test_status_text(tmp_path):
    src, exe = tmp_path / "status.cpp", tmp_path / "status"
    src.write_text(STATUS_PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc", "binding"), "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines() == [
        "op: HIP call failed: flownet2_hip_sample1d: invalid shape or parameter (1 .. 8 levels, radius 0 .. 8, a coords batch stride of at least H W)"
        " (code -1)",
        "op: HIP call failed: flownet2_hip_sample1d: unknown error (code -2)",
        "op: HIP call failed: flownet2_hip_sample1d: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_sample1d: unsupported size (2^31 query pixels or more, or a level beyond 2^48 cells) (code -4)",
        "op: HIP call failed: flownet2_hip_sample1d: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_sample1d: unknown error (code -9)"]


def test_binding_refuses_with_the_argument_and_the_remedy():
    import corr_sample1d_cuda
    from networks.correlation_package import CorrBlock1D, CorrSample1d, corr_sample1d
    pyr, co = [torch.zeros(8, 1, 1, 4), torch.zeros(8, 1, 1, 2)], torch.zeros(1, 2, 2, 4)
    with pytest.raises(RuntimeError, match="coords must be a GPU .HIP. tensor; this extension has no CPU implementation"):
        corr_sample1d_cuda.forward_alloc(pyr, co, 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_sample1d_cuda.backward_alloc(co, torch.zeros(1, 10, 2, 4), [4, 2], [4, 4], 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_sample1d(pyr, co[:, :1], 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        CorrBlock1D(torch.zeros(1, 4, 2, 4), torch.zeros(1, 4, 2, 4), num_levels=2, radius=2)(co)
    with pytest.raises(RuntimeError, match=r"pass coords\.detach\(\)"):   # before anything else: a silent None would train wrongly
        corr_sample1d(pyr, co.clone().requires_grad_(True), 2)
    # the checks that come before the device's: dtype, counts, shapes -- each names the argument and the remedy
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(RuntimeError, match=r"coords must be float32, got .*: convert it with \.float\(\)"):
            torch.ops.fn2.corr_sample1d([t.to(META) for t in pyr], co.to(META).to(dt), 2)
    with pytest.raises(ValueError, match="num_levels 4 leaves an empty level for fmap2 of width 4: use at most 3 levels"):
        CorrBlock1D(torch.zeros(1, 4, 2, 4), torch.zeros(1, 4, 2, 4), num_levels=4, radius=2)
    assert len(CorrBlock1D(torch.zeros(1, 4, 2, 5), torch.zeros(1, 4, 2, 4), num_levels=3, radius=2).corr_pyramid) == 3
    assert "radius=3" in repr(CorrSample1d(3))


# ------------------------------------------------------------------ the operators
_LISTINGS = """
import importlib, sys
import torch, fn2_ops
for m in ("networks.census_package.census", "networks.correlation_package.corr_block", "networks.correlation_package.corr_pyramid",
          "networks.ssim_package.ssim"):
    importlib.import_module(m)
before = (fn2_ops.names(), fn2_ops.names(preview=True), fn2_ops.names(incubating=True), fn2_ops.names(staging=True))
assert all(before) and not any("corr_sample1d" in n for names in before for n in names)
ext = {m for m in sys.modules if m.endswith("_cuda")}
importlib.import_module("networks.correlation_package.corr_block1d")
assert (fn2_ops.names(), fn2_ops.names(preview=True), fn2_ops.names(incubating=True)) == before[:3]
gained = sorted(set(fn2_ops.names(staging=True)) - set(before[3]))
assert gained == ["fn2::corr_sample1d", "fn2::corr_sample1d_backward"] and set(before[3]) <= set(fn2_ops.names(staging=True)), gained
assert not set(gained) & set(before[0] + before[1] + before[2])
assert {m for m in sys.modules if m.endswith("_cuda")} - ext == {"corr_sample1d_cuda"}
print("listed")
"""

_ALONE = """
import importlib, sys
import torch, fn2_ops
import networks.correlation_package as P
assert not [m for m in sys.modules if m.endswith("_cuda")]
assert P.CorrBlock1D.__name__ == "CorrBlock1D" and callable(P.corr_sample1d) and P.CorrSample1d and P.CorrSample1dFunction
assert {m for m in sys.modules if m.endswith("_cuda")} == {"corr_sample1d_cuda"}
assert fn2_ops.names(staging=True) == ["fn2::corr_sample1d", "fn2::corr_sample1d_backward"]
assert fn2_ops.names() == fn2_ops.names(preview=True) == fn2_ops.names(incubating=True) == []
print("alone")
"""


@pytest.mark.parametrize("script, word", [(_LISTINGS, "listed"), (_ALONE, "alone")], ids=["after the others", "alone"])
def test_staging_operators_are_in_no_other_listing(script, word):
    code = "import sys; sys.path[:0] = %r\n" % [PKG, ROOT] + script
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert res.returncode == 0 and word in res.stdout, res.stderr[-2000:]


def test_nothing_existing_imports_the_new_module():
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py") and f != "corr_block1d.py":
                text = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s.*(corr_block1d|corr_sample1d_cuda)", text, flags=re.M), os.path.join(d, f)
                if f not in ("__init__.py", "fn2_capi.py"):        # (the lazy export table; a comment on the library)
                    assert "corr_block1d" not in text, os.path.join(d, f)


def _compile(fn, **kw):
    import torch._dynamo
    torch._dynamo.reset()
    return torch.compile(fn, backend="aot_eager", fullgraph=True, **kw)


def _t(*shape, dtype=torch.float32, grad=False):
    return torch.empty(*shape, dtype=dtype, device=META, requires_grad=grad)


def _block(fmap1, fmap2, coords):
    from networks.correlation_package import CorrBlock1D
    return CorrBlock1D(fmap1, fmap2, num_levels=3, radius=2)(coords)


@pytest.mark.parametrize("channels", [2, 1])
def test_corr_block1d_traces_forward_and_backward(channels):
    import torch._dynamo
    a, b, c = _t(2, 8, 9, 11, grad=True), _t(2, 8, 9, 13, grad=True), _t(2, channels, 9, 11)
    out = _compile(_block)(a, b, c)
    assert tuple(out.shape) == (2, 15, 9, 11) and out.dtype == torch.float32 and out.requires_grad and out.is_contiguous()
    g1, g2 = torch.autograd.grad(out.sum(), (a, b))
    assert g1.shape == a.shape and g2.shape == b.shape
    torch._dynamo.reset()
    rep = torch._dynamo.explain(_block)(a, b, c)
    assert rep.graph_break_count == 0 and rep.graph_count == 1, rep.break_reasons
    out = _compile(_block)(a.half(), b.half(), c.double())         # RAFT-Stereo's .float() on the maps and the coordinates
    assert out.dtype == torch.float32


def test_opcheck_schema_and_fake():
    import networks.correlation_package.corr_block1d  # noqa: F401
    pyr = [_t(198, 1, 1, 11, grad=True), _t(198, 5, grad=True)]
    co = _t(2, 2, 9, 11)
    for op, args in ((torch.ops.fn2.corr_sample1d, (pyr, co, 2)), (torch.ops.fn2.corr_sample1d_backward, (co, _t(2, 10, 9, 11), [11, 5], [4, 2], 2))):
        res = torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
        assert set(res.values()) == {"SUCCESS"}, res
    assert tuple(torch.ops.fn2.corr_sample1d(pyr, co[:, :1], 2).shape) == (2, 10, 9, 11)
    grads = torch.ops.fn2.corr_sample1d_backward(co, _t(2, 10, 9, 11), [11, 5], [4, 2], 2)       # the levels' shapes, not the levels
    assert [tuple(g.shape) for g in grads] == [(198, 1, 1, 11), (198, 5)] and all(g.dtype == torch.float32 for g in grads)


def test_backward_operator_is_not_differentiable_twice():
    import networks.correlation_package.corr_block1d  # noqa: F401
    go = _t(2, 5, 9, 11, grad=True)
    g, = torch.ops.fn2.corr_sample1d_backward(_t(2, 2, 9, 11), go, [11], [4], 2)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="fn2::corr_sample1d_backward: the backward of this layer is a HIP kernel and not differentiable a second time"):
        g.sum().backward()


def _refusals():
    from networks.correlation_package import CorrSample1d, corr_sample1d
    pyr, co = [_t(198, 1, 1, 11, grad=True), _t(198, 1, 1, 5)], _t(2, 2, 9, 11)
    return {
        "radius": (CorrSample1d(9), (pyr, co), "radius 9 outside 0 .. 8"),
        "half pyramid": (CorrSample1d(3), ([t.half() for t in pyr], co), r"float32 tensors expected, got torch.float16 .*use \.float\(\)"),
        "half coords": (CorrSample1d(3), (pyr, co.half()), r"coords must be float32, got torch.float16: convert it with \.float\(\)"),
        "coords grad": (CorrSample1d(3), (pyr, _t(2, 2, 9, 11, grad=True)), r"coords requires grad.*pass coords\.detach\(\)"),
        "coords channels": (CorrSample1d(3), (pyr, _t(2, 3, 9, 11)), r"coords has shape \(2, 3, 9, 11\), expected \[B, 2, H, W\]"),
        "first dimension": (CorrSample1d(3), (pyr, _t(2, 2, 9, 12)), r"a pyramid level has shape \(198, 1, 1, 11\), expected \[216, 1, 1, W2\]"),
        "2-D level": (CorrSample1d(3), ([_t(198, 1, 3, 11)], co), r"a pyramid level has shape \(198, 1, 3, 11\), expected \[198, 1, 1, W2\] or \[198, W2\]"),
        "no levels": (lambda c: corr_sample1d([], c, 3), (co,), "the pyramid has 0 levels, expected 1 .. 8"),
        "nine levels": (lambda c: corr_sample1d([_t(198, 4)] * 9, c, 3), (co,), "the pyramid has 9 levels, expected 1 .. 8"),
    }


@pytest.mark.parametrize("which", ["radius", "half pyramid", "half coords", "coords grad", "coords channels", "first dimension", "2-D level",
                                   "no levels", "nine levels"])
def test_refused_at_trace_time(which):
    fn, args, match = _refusals()[which]
    with pytest.raises(Exception, match=match):
        _compile(fn)(*args)
    if which == "coords grad":
        return
    op_args = (args[0], args[1], fn.radius) if hasattr(fn, "radius") else ([] if which == "no levels" else [_t(198, 4)] * 9, args[0], 3)
    with pytest.raises(RuntimeError, match="fn2::corr_sample1d: .*" + match):      # ... and by the operator called directly
        torch.ops.fn2.corr_sample1d(*op_args)
    if which in ("half pyramid", "first dimension", "2-D level"):
        return          # the backward operator takes the levels' shapes, not the levels: nothing of a level is left to refuse
    levels, co, radius = op_args
    go = _t(2, max(len(levels), 1) * (2 * radius + 1), 9, 11)
    with pytest.raises(RuntimeError, match="fn2::corr_sample1d_backward: .*" + match):
        torch.ops.fn2.corr_sample1d_backward(co, go, [t.shape[-1] for t in levels], [t.dim() for t in levels], radius)


def test_backward_operator_refuses_bad_shapes_of_its_own():
    import networks.correlation_package.corr_block1d  # noqa: F401
    co, go = _t(2, 2, 9, 11), _t(2, 10, 9, 11)
    for widths, dims, match in (([11, 5], [4], "2 widths but 1 dims"), ([11, 5], [4, 3], "level 1 has 3 dimensions, expected 2 .* or 4"),
                                ([11, 0], [4, 2], "level 1 is 0 cells wide, expected at least 1")):
        with pytest.raises(RuntimeError, match="fn2::corr_sample1d_backward: " + match):
            torch.ops.fn2.corr_sample1d_backward(co, go, widths, dims, 2)
    with pytest.raises(RuntimeError, match=r"gradOutput has shape \(2, 9, 9, 11\), expected \[2, 10, 9, 11\]"):
        torch.ops.fn2.corr_sample1d_backward(co, _t(2, 9, 9, 11), [11, 5], [4, 2], 2)


def test_static_forward_refuses_coords_that_require_grad_eagerly_too():
    """Driving the Function's static methods outside torch.compile: no silent None for coords there either."""
    from networks.correlation_package import CorrSample1dFunction
    pyr, co = [torch.zeros(8, 1, 1, 4, requires_grad=True)], torch.zeros(1, 2, 2, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match=r"coords requires grad.*pass coords\.detach\(\)"):
        super(CorrSample1dFunction, CorrSample1dFunction).apply(co, 2, *pyr)


def test_the_bindings_checks_on_cpu_tensors_match_the_operators():
    """The binding's own wording, reached with CPU tensors where the check comes before the device's (coords is looked at first)."""
    import corr_sample1d_cuda
    lv = [torch.zeros(8, 1, 1, 4)]
    with pytest.raises(RuntimeError, match=r"corr_sample1d_cuda.forward: coords must be a GPU"):
        corr_sample1d_cuda.forward_alloc(lv, torch.zeros(1, 2, 2, 4), 9)
