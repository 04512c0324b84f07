"""CPU-side checks of the incubating library libflownet2_hip_pyramid.so (include/preview/flownet2_hip_pyramid.h; CorrPyramid).

The float64 reference (tests/corr_pyramid_ref.py) against RAFT's composition, values and both gradients; the bound is reachable (the
float32 composition stays inside it) and has teeth (five mutations of the reference miss it); the incubating record -- exports ==
header == fn2_capi, ABI version 0, nothing linked, the three tables of build.py disjoint and the released ones unchanged, the header
compiles as C99 in every order the other headers allow; every rejection in front of a launch and its order (host pointers, no GPU);
STATUS_PYRAMID's texts; the operators on the meta device, refusals at trace time; CorrBlock's switch."""
import ctypes
import os
import subprocess
import sys
import sysconfig
import types

import pytest
import torch

from conftest import PKG, ROOT

import build
import corr_pyramid_ref as RP
import fn2_capi
from test_corr_sample_host import RELEASED_HEADERS
from test_libraries_host import _declared, _exported, _needed

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
NAMES = ["fn2y_abi_version", "fn2y_corr_pyramid_fold", "fn2y_corr_pyramid_forward"]
META = torch.device("meta")
_CACHE = {}


def _reference(shape):
    if shape not in _CACHE:
        f1, f2 = RP.inputs(shape, seed=5)
        levels, S0 = RP.forward(f1, f2, shape[4])
        _CACHE[shape] = (f1, f2, levels, S0, RP.bounds(levels, S0, shape[1]))
    return _CACHE[shape]


def _grads(shape, seed):
    B, C, (H, W), (H2, W2), L = shape
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B * H * W, 1, H2 >> l, W2 >> l, generator=g) for l in range(L)]


# ------------------------------------------------------------------ the reference and the bound
@pytest.mark.parametrize("shape", RP.SHAPES, ids=RP.shape_id)
def test_reference_against_rafts_composition(shape):
    """Values and both gradients (autograd through matmul / sqrt(C) and avg_pool2d) to 1e-12 relative, in float64."""
    B, C, (H, W), (H2, W2), L = shape
    f1, f2, levels, S0, _ = _reference(shape)
    assert [tuple(t.shape[1:]) for t in levels] == RP.level_sizes(H2, W2, L) == [(H2 >> l, W2 >> l) for l in range(L)]
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    pyr = RP.composition(a, b, L)
    for l, (t, w) in enumerate(zip(pyr, levels)):
        assert tuple(t.shape) == (B * H * W, 1) + tuple(w.shape[1:])
        assert float((t[:, 0] - w).abs().max()) <= 1e-12 * float(w.abs().max()), l
    assert bool((S0 >= levels[0].abs() * (1 - 1e-12)).all())
    gouts = _grads(shape, 9)
    w1, w2 = torch.autograd.grad(pyr, (a, b), [g.double() for g in gouts])
    G, g1, g2 = RP.backward(f1, f2, gouts)
    assert tuple(G.shape) == (B * H * W, H2, W2)
    for g, w in ((g1, w1), (g2, w2)):
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())
    # a missing gradient counts as zero
    some = list(gouts)
    some[0] = None
    if L > 1:
        _, m1, _ = RP.backward(f1, f2, some)
        z1, _ = torch.autograd.grad(RP.composition(a, b, L)[1:], (a, b), [g.double() for g in gouts[1:]])
        assert float((m1 - z1).abs().max()) <= 1e-12 * float(z1.abs().max())


@pytest.mark.parametrize("shape", RP.SHAPES, ids=RP.shape_id)
def test_the_bound_is_reachable(shape):
    """The float32 PyTorch composition on the CPU stays inside delta_l."""
    f1, f2, levels, _, deltas = _reference(shape)
    got = RP.composition(f1, f2, shape[4])
    worst, per = RP.worst_ratio(got, levels, deltas)
    print(f"  {RP.shape_id(shape)}: float32 composition, error / bound per level " + " ".join(f"{r:.4f}" for r in per))
    assert not RP.misses(got, levels, deltas), worst


@pytest.mark.parametrize("mutation", RP.MUTATIONS)
def test_the_bound_has_teeth(mutation):
    """Each mistake, made in the float64 reference itself, misses delta_l somewhere (or has levels of another shape)."""
    hit = []
    for shape in RP.SHAPES:
        B, C, (H, W), (H2, W2), L = shape
        f1, f2, levels, S0, deltas = _reference(shape)
        if mutation == "fold_weight":
            if L < 3:
                continue
            gouts = _grads(shape, 3)
            G, g1, g2 = RP.backward(f1, f2, gouts)
            Gm, m1, m2 = RP.backward(f1, f2, gouts, mutation)
            # the fold's own tolerance: three rounded adds and a product, 4 * 2^-24 of the sum of the absolute terms
            tol = 4 * 2.0 ** -24 * RP.fold([g.double().abs() for g in gouts], C, H2, W2)
            assert bool(((Gm - G).abs() > tol).any())
            e1 = _rule_bound(g1, f1, f2, gouts, "fmap1.grad")
            assert float((m1 - g1).abs().max()) > e1
            hit.append(shape)
            continue
        if (mutation in ("ceil", "pool_half") and L < 2):
            continue
        mutated, _ = RP.forward(f1, f2, L, mutation)
        if mutation == "ceil" and all(h % 2 == 0 and w % 2 == 0 for h, w in RP.level_sizes(H2, W2, L)[:-1]):
            assert not RP.misses(mutated, levels, deltas)     # nothing ragged: ceil and floor agree
            continue
        assert RP.misses(mutated, levels, deltas), RP.shape_id(shape)
        hit.append(shape)
    assert hit, mutation
    if mutation == "swap":
        assert any(s[2] != s[3] for s in hit) and any(s[2] == s[3] for s in hit)


def _rule_bound(g64, f1, f2, gouts, key):
    """The bound of the gradient rule (tests/pipelines_ref.py) for one gradient: from the float32 composition's own error."""
    import pipelines_ref as P
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    torch.autograd.backward(RP.composition(a, b, len(gouts)), gouts)
    return P.rule_bound({"fmap1.grad": a.grad, "fmap2.grad": b.grad}[key], g64)


def test_restatements():
    """pool32 and fold32 are float32 and agree with the float64 formulas to rounding; the fold leaves a cropped level's cells alone."""
    shape = RP.SHAPES[2]
    B, C, (H, W), (H2, W2), L = shape
    f1, f2, levels, S0, deltas = _reference(shape)
    lvl = levels[0].float()
    for l in range(1, L):
        nxt = RP.pool32(lvl)
        assert nxt.dtype == torch.float32 and float((nxt.double() - RP.pool_exact(lvl.double())).abs().max()) <= 3 * 2.0 ** -24 * float(S0.max())
        lvl = nxt
    gouts = _grads(shape, 4)
    G32, G64 = RP.fold32(gouts, C, H2, W2), RP.fold([g.double() for g in gouts], C, H2, W2)
    assert G32.dtype == torch.float32
    assert bool(((G32.double() - G64).abs() <= 5 * 2.0 ** -24 * RP.fold([g.double().abs() for g in gouts], C, H2, W2)).all())
    one = [torch.zeros_like(g) for g in gouts]
    one[3][0, 0, 1, 3] = 1.0             # level 3 of 17 x 35 is 2 x 4: rows 8 .. 15, columns 24 .. 31; row 16 and columns 32 .. 34 get nothing
    nz = RP.fold32(one, C, H2, W2).nonzero()
    assert len(nz) == 64 and int(nz[:, 1].min()) == 8 and int(nz[:, 1].max()) == 15 and int(nz[:, 2].min()) == 24 and int(nz[:, 2].max()) == 31
    assert float(RP.fold32(one, C, H2, W2).max()) == float(torch.tensor(1 / 64.0) * torch.tensor(C ** -0.5, dtype=torch.float64).float())


# ------------------------------------------------------------------ the incubating record
def test_incubating_table_and_the_other_records():
    assert list(build.INCUBATING) == ["pyramid"]
    desc = build.INCUBATING["pyramid"]
    assert desc.srcs == ["capi_pyramid.hip", "corr_pyramid.hip"] and desc.modules == ["corr_pyramid_cuda"]
    assert desc.link == "flownet2_hip_pyramid" and desc.vmap == "exports_pyramid.map" and desc.header == "preview/flownet2_hip_pyramid.h"
    assert type(desc) is type(build.LIBRARIES[""])
    assert len(build.LIBRARIES) == 7 and len(build.MODULES) == 10 and list(build.PREVIEW) == ["sample"]
    tables = (build.LIBRARIES, build.PREVIEW, build.INCUBATING)
    assert build.TABLES == tables and sum(len(t) for t in tables) == len(set().union(*tables)) == 9
    assert "corr_pyramid_cuda" not in build.MODULES and "corr_pyramid_cuda" not in build.PREVIEW["sample"].modules
    assert build._described("pyramid") is desc and build._described("sample") is build.PREVIEW["sample"] and build._described("") is build.LIBRARIES[""]
    assert sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h")) == sorted(RELEASED_HEADERS)
    assert sorted(os.listdir(os.path.join(ROOT, "include", "preview"))) == ["flownet2_hip_pyramid.h", "flownet2_hip_sample.h"]


def test_library_exports_what_its_header_declares():
    desc = build.INCUBATING["pyramid"]
    path = fn2_capi.PYRAMID_LIB_PATH
    assert os.path.samefile(path, os.path.join(PKG, "lib", "lib%s.so" % desc.link))
    m = RP.header_macros()
    assert fn2_capi.pyramid_lib().fn2y_abi_version() == 0 == m["FN2Y_ABI_VERSION"]
    assert m["FN2Y_MAX_LEVELS"] == fn2_capi.FN2Y_MAX_LEVELS == 4
    assert (m["FN2Y_TILE_QUERIES"], m["FN2Y_TILE_ROWS"], m["FN2Y_TILE_COLS"]) == (128, 8, 32)
    assert m["FN2Y_BOUND_SPLIT"] == 2 * 2.0 ** -24 + 2.0 ** -32 and m["FN2Y_BOUND_PER_CHANNEL"] == 6 * 2.0 ** -23 * (1 + 2.0 ** -7)
    assert m["FN2Y_BOUND_PER_POOL"] == 3 * 2.0 ** -23
    assert _exported(path) == _declared(desc.header, "fn2y_") == sorted(fn2_capi.PYRAMID_EXPORTS) == NAMES
    assert _needed(path) == []
    # no other library, the debug twin included, exports an fn2y_ name
    for table in (build.LIBRARIES, build.PREVIEW):
        for name in table:
            stem = name.upper() + "_" if name else ""
            assert not any(n.startswith("fn2y_") for n in getattr(fn2_capi, stem + "EXPORTS")), name
            assert not any(n.startswith("fn2y_") for n in _exported(getattr(fn2_capi, stem + "LIB_PATH"))), name
    assert not any(n.startswith("fn2y_") for n in fn2_capi.DEBUG_EXPORTS)


def test_module_links_exactly_its_library():
    assert _needed(os.path.join(PKG, "corr_pyramid_cuda" + sysconfig.get_config_var("EXT_SUFFIX"))) == ["libflownet2_hip_pyramid.so"]
    text = open(os.path.join(PKG, "csrc", "binding", "corr_pyramid_cuda.cpp")).read()
    assert "STATUS_PYRAMID" in text and "fn2_strerror(" not in text
    for table in (build.LIBRARIES, build.PREVIEW):
        for lib in table.values():
            for module in lib.modules:
                assert "STATUS_PYRAMID" not in open(os.path.join(PKG, "csrc", "binding", module + ".cpp")).read(), module


def test_header_compiles_alone_and_after_the_others(tmp_path):
    # by itself; after all seven released headers in their documented order; after each of them; after the sample preview header;
    # after everything
    sample = "preview/flownet2_hip_sample.h"
    orders = [[], RELEASED_HEADERS, [sample], RELEASED_HEADERS + [sample]] + [[h] for h in RELEASED_HEADERS]
    for i, incs in enumerate(orders):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in list(incs) + ["preview/flownet2_hip_pyramid.h"]) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2Y_MAX_LEVELS + FN2Y_TILE_ROWS + FN2Y_ABI_VERSION];\n"
                       "double bound = FN2Y_BOUND_SPLIT + 256 * FN2Y_BOUND_PER_CHANNEL + 3 * FN2Y_BOUND_PER_POOL;\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ rejections
def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.pyramid_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 2)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*[x.value for x in v])

    def fwd(a, b, levels, L, B, C, H, W, H2, W2):
        return lib.fn2y_corr_pyramid_forward(a, b, levels, L, B, C, H, W, H2, W2, null)

    def fold(G, _, levels, L, B, C, H, W, H2, W2):
        return lib.fn2y_corr_pyramid_fold(levels, L, G, B, C, H, W, H2, W2, null)

    good = ptrs(p, p)
    for call in (fwd, fold):
        # 1. parameters and sizes, whatever else is wrong
        for L in (0, -1, 5):
            assert call(null, null, None, L, 1, 8, 8, 16, 8, 16) == EINVAL, L
        for B, C, H, W, H2, W2 in ((-1, 8, 8, 16, 8, 16), (1, 0, 8, 16, 8, 16), (1, 8, 0, 16, 8, 16), (1, 8, 8, 0, 8, 16), (1, 8, 8, 16, 0, 16),
                                   (1, 8, 8, 16, 8, -1)):
            assert call(null, null, None, 2, B, C, H, W, H2, W2) == EINVAL, (B, C, H, W, H2, W2)
        assert call(null, null, None, 4, 1, 8, 8, 16, 7, 16) == EINVAL             # 7 >> 3 == 0: an empty level
        assert call(null, null, None, 2, 1, 8, 8, 16, 8, 1) == EINVAL
        assert call(null, null, None, 4, 1, 8, 65536, 65536, 7, 16) == EINVAL       # sizes before the limits
        assert call(null, null, None, 3, 1, 8, 8, 16, 7, 16) == EINVAL              # 7 >> 2 == 1: passes, to check 4
        # 2. limits
        assert call(null, null, None, 2, 1, 8, 65536, 32768, 8, 16) == EUNSUPPORTED
        assert call(null, null, None, 2, 4, 8, 32768, 16384, 8, 16) == EUNSUPPORTED
        assert call(null, null, None, 2, 1, 8, 8, 16, 65536, 32768) == EUNSUPPORTED
        assert call(null, null, None, 2, 1, 8, 1024, 1025, 16384, 16384) == EUNSUPPORTED     # (2^20 + 2^10) 2^28 cells
        assert call(null, null, None, 2, 1, (1 << 20) + 1, 8, 16, 8, 16) == EUNSUPPORTED
        assert call(null, null, None, 2, 0, 8, 65536, 32768, 8, 16) == EUNSUPPORTED          # limits before the empty batch
        # 3. the empty batch: nothing to do, whatever the pointers
        assert call(null, null, None, 2, 0, 8, 8, 16, 8, 16) == OK
        assert call(mis, null, ptrs(mis, null), 2, 0, 8, 8, 16, 8, 16) == OK
        # 4. NULL, also next to a misaligned pointer: NULL is reported first
        assert call(p, p, None, 2, 1, 8, 8, 16, 8, 16) == EINVAL
        assert call(null, p, ptrs(mis, p), 2, 1, 8, 8, 16, 8, 16) == EINVAL
        # 5. alignment to 4 bytes
        assert call(mis, p, good, 2, 1, 8, 8, 16, 8, 16) == EALIGN
        assert call(p, p, ptrs(p, mis), 2, 1, 8, 8, 16, 8, 16) == EALIGN
        assert call(p, p, ptrs(mis, p), 2, 1, 8, 8, 16, 8, 16) == EALIGN
    assert fwd(p, null, good, 2, 1, 8, 8, 16, 8, 16) == EINVAL
    assert fwd(p, mis, good, 2, 1, 8, 8, 16, 8, 16) == EALIGN
    assert fwd(p, p, ptrs(p, null), 2, 1, 8, 8, 16, 8, 16) == EINVAL        # every level of the forward is required ...
    assert fwd(mis, p, ptrs(null, p), 2, 1, 8, 8, 16, 8, 16) == EINVAL
    assert fold(mis, None, ptrs(null, p), 2, 1, 8, 8, 16, 8, 16) == EALIGN      # ... a missing gradient of the fold is not
    # 6. the forward's grid: 2^48 cells pass checks 1 - 5 and are 2^33 workgroups
    assert fwd(p, p, ptrs(p), 1, 1, 8, 1024, 1024, 16384, 16384) == EUNSUPPORTED


STATUS_PROGRAM = """
#include <cstdio>
#include "binding_status.h"
int main()
{
    const int codes[] = {-1, -2, -3, -4, 7, -9};
    for (int rc : codes) std::puts(fn2b::status_message(fn2b::STATUS_PYRAMID, "op", rc).c_str());
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
        "op: HIP call failed: flownet2_hip_pyramid: invalid shape, layout or parameter (contiguous maps, 1 .. 4 levels, none of them empty) (code -1)",
        "op: HIP call failed: flownet2_hip_pyramid: dtype not supported by this op (float32 only: convert with .float()) (code -2)",
        "op: HIP call failed: flownet2_hip_pyramid: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_pyramid: unsupported size (2^31 query pixels or more, a slice of 2^31 cells or more, a volume beyond 2^48 "
        "cells, more than 2^20 channels, or 2^31 workgroups or more) (code -4)",
        "op: HIP call failed: flownet2_hip_pyramid: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_pyramid: unknown error (code -9)"]
    # the fake implementations say the same
    import networks.correlation_package.corr_pyramid as M
    assert M._status("op", M._EINVAL, -1) == lines[0] and M._status("op", M._EDTYPE, -2) == lines[1]


def test_cpu_tensors_are_refused():
    import corr_pyramid_cuda
    from networks.correlation_package import CorrBlock, corr_pyramid
    a, b = torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_pyramid_cuda.forward_alloc(a, b, 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_pyramid_cuda.backward_alloc(a, b, [torch.zeros(64, 1, 8, 8), None])
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_pyramid(a, b, 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        CorrBlock(a, b, num_levels=2, radius=2, fused_build=True)


# ------------------------------------------------------------------ torch.compile and the operators
def _compile(fn, **kw):
    import torch._dynamo
    torch._dynamo.reset()
    return torch.compile(fn, backend="aot_eager", fullgraph=True, **kw)


def _t(*shape, dtype=torch.float32, grad=False):
    return torch.empty(*shape, dtype=dtype, device=META, requires_grad=grad)


def test_opcheck_schema_and_fake():
    import fn2_ops
    before = (fn2_ops.names(), fn2_ops.names(preview=True))
    import networks.correlation_package.corr_pyramid  # noqa: F401
    a, b = _t(2, 8, 9, 11, grad=True), _t(2, 8, 17, 35, grad=True)
    grads = [_t(198, 1, 17, 35), None, _t(198, 1, 4, 8)]
    for op, args in ((torch.ops.fn2.corr_pyramid, (a, b, 3)), (torch.ops.fn2.corr_pyramid_backward, (a, b, grads))):
        res = torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
        assert set(res.values()) == {"SUCCESS"}, res
    out = torch.ops.fn2.corr_pyramid(a, b, 3)
    assert [tuple(t.shape) for t in out] == [(198, 1, 17, 35), (198, 1, 8, 17), (198, 1, 4, 8)] and all(t.is_contiguous() for t in out)
    g1, g2 = torch.ops.fn2.corr_pyramid_backward(a, b, grads)
    assert g1.shape == a.shape and g2.shape == b.shape
    g1, g2 = torch.autograd.grad([out[0].sum(), out[2].sum()], (a, b))
    assert g1.shape == a.shape and g2.shape == b.shape
    # the incubating operators have a listing of their own; the other two are what they were
    assert fn2_ops.names(incubating=True) == ["fn2::corr_pyramid", "fn2::corr_pyramid_backward"]
    assert (fn2_ops.names(), fn2_ops.names(preview=True)) == before
    assert not any("corr_pyramid" in n for n in before[0] + before[1])


def test_backward_operator_is_not_differentiable_twice():
    import networks.correlation_package.corr_pyramid  # noqa: F401
    g1, _ = torch.ops.fn2.corr_pyramid_backward(_t(2, 8, 9, 11), _t(2, 8, 9, 11), [_t(198, 1, 9, 11, grad=True)])
    assert g1.requires_grad
    with pytest.raises(RuntimeError, match="not differentiable a second time"):
        g1.sum().backward()


def test_corr_pyramid_traces_forward_and_backward():
    import torch._dynamo
    from networks.correlation_package.corr_pyramid import CorrPyramid, corr_pyramid

    def fn(x, y):
        return corr_pyramid(x, y, 5)

    a, b = _t(2, 8, 9, 11, grad=True), _t(2, 8, 32, 48, grad=True)
    out = _compile(fn)(a, b)
    assert [tuple(t.shape) for t in out] == [(198, 1, 32 >> l, 48 >> l) for l in range(5)] and all(t.requires_grad for t in out)
    g1, g2 = torch.autograd.grad(sum(t.sum() for t in out), (a, b))
    assert g1.shape == a.shape and g2.shape == b.shape
    torch._dynamo.reset()
    rep = torch._dynamo.explain(fn)(a, b)
    assert rep.graph_break_count == 0 and rep.graph_count == 1, rep.break_reasons
    assert len(_compile(CorrPyramid(2))(a, b)) == 2


def _refusals():
    from networks.correlation_package.corr_pyramid import CorrPyramid
    a, b = _t(2, 8, 9, 11), _t(2, 8, 9, 11)
    return {
        "no levels": (CorrPyramid(0), (a, b), "invalid shape, layout or parameter"),
        "empty level": (CorrPyramid(4), (a, _t(2, 8, 7, 11)), "invalid shape, layout or parameter"),
        "half maps": (CorrPyramid(2), (a.half(), b.half()), "dtype not supported by this op"),
        "mixed dtypes": (CorrPyramid(2), (a, b.half()), "fmap2 has dtype"),
        "channels": (CorrPyramid(2), (a, _t(2, 4, 9, 11)), r"must be \[B, C, H, W\]"),
        "not contiguous": (CorrPyramid(2), (_t(2, 8, 11, 9).transpose(2, 3), b), "invalid shape, layout or parameter"),
    }


@pytest.mark.parametrize("which", ["no levels", "empty level", "half maps", "mixed dtypes", "channels", "not contiguous"])
def test_refused_at_trace_time(which):
    fn, args, match = _refusals()[which]
    with pytest.raises(Exception, match=match):
        _compile(fn)(*args)


# ------------------------------------------------------------------ CorrBlock's switch
def test_default_corr_block_does_not_load_the_extension():
    code = ("import sys, torch\n"
            "from networks.correlation_package import CorrBlock\n"
            "b = CorrBlock(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8), num_levels=2, radius=1)\n"
            "assert [tuple(t.shape) for t in b.corr_pyramid] == [(64, 1, 8, 8), (64, 1, 4, 4)]\n"
            "assert 'corr_pyramid_cuda' not in sys.modules and 'networks.correlation_package.corr_pyramid' not in sys.modules\n"
            "try:\n"
            "    CorrBlock(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8), num_levels=2, radius=1, fused_build=True)\n"
            "except RuntimeError as e:\n"
            "    assert 'no CPU implementation' in str(e)\n"
            "assert 'corr_pyramid_cuda' in sys.modules\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr


def test_mini_raft_with_fused_build_traces():
    import torch._dynamo

    import compile_cases as CC
    import pipelines_ref as P
    from networks.correlation_package import CorrBlock
    layers = types.SimpleNamespace(**{**vars(P.hip_layers()),
                                      "corr_block": lambda f1, f2, L, r: CorrBlock(f1, f2, num_levels=L, radius=r, fused_build=True)})
    meta = {k: torch.empty(v.shape, dtype=torch.float32, device=META) for k, v in P.raft_inputs().items()}
    out = CC.run_mini_raft(_compile(CC.mini_raft_forward), layers, meta)
    N, H, W = P.RAFT_SHAPE
    assert all(out["flow_up_%d" % i].shape == (N, 2, H, W) for i in range(P.RAFT_ITERS)) and out["loss"].shape == ()
    assert out["fmap1.grad"].shape == out["fmap2.grad"].shape == (N, P.RAFT_CHANNELS, H // 8, W // 8)
    torch._dynamo.reset()
    params = {k: meta[k].detach().clone().requires_grad_(True) for k in P.RAFT_PARAMS}
    fmap = torch.empty((N, P.RAFT_CHANNELS, H // 8, W // 8), device=META, requires_grad=True)
    rep = torch._dynamo.explain(CC.mini_raft_forward)(layers, meta, params, fmap, fmap.clone(), None)
    assert rep.graph_break_count == 0 and rep.graph_count == 1, rep.break_reasons
