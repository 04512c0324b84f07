"""CPU-side checks of the preview library libflownet2_hip_sample.so (include/preview/flownet2_hip_sample.h; CorrSample / CorrBlock).

The preview record, as tests/test_libraries_host.py keeps it for the seven released libraries: exports == header == fn2_capi == the
names written out here, ABI version 0, no project library linked, the module links exactly its library, no released library exports
an fn2p_ name, build.LIBRARIES / build.MODULES unchanged, the header compiles after all seven released headers.  Then every
rejection in front of a launch and its order (host pointers, no GPU), STATUS_SAMPLE's text, the float64 reference against RAFT's
all-pairs + grid_sample composition (values and both feature-map gradients), the channel and level order, and torch.compile /
torch.library over the operators on the meta device, refusals at trace time included."""
import ctypes
import os
import re
import subprocess
import sysconfig
import types

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

import build
import corr_lookup_ref as RL
import corr_sample_ref as RS
import fn2_capi
from test_libraries_host import _declared, _exported, _needed

OK, EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
NAMES = ["fn2p_abi_version", "fn2p_corr_sample_backward", "fn2p_corr_sample_forward"]
RELEASED_HEADERS = ["flownet2_hip.h", "flownet2_hip_ext.h", "flownet2_hip_lookup.h", "flownet2_hip_upsample.h", "flownet2_hip_splat.h",
                    "flownet2_hip_census.h", "flownet2_hip_smooth.h"]
META = torch.device("meta")


# ------------------------------------------------------------------ the preview record
def test_preview_table_and_the_released_record():
    assert list(build.PREVIEW) == ["sample"]
    desc = build.PREVIEW["sample"]
    assert desc.srcs == ["capi_sample.hip", "corr_sample.hip"] and desc.modules == ["corr_sample_cuda"]
    assert desc.link == "flownet2_hip_sample" and desc.vmap == "exports_sample.map" and desc.header == "preview/flownet2_hip_sample.h"
    assert type(desc) is type(build.LIBRARIES[""])
    assert len(build.LIBRARIES) == 7 and len(build.MODULES) == 10
    assert "sample" not in build.LIBRARIES and "corr_sample_cuda" not in build.MODULES
    assert sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h")) == sorted(RELEASED_HEADERS)


def test_library_exports_what_its_header_declares():
    desc = build.PREVIEW["sample"]
    path = fn2_capi.SAMPLE_LIB_PATH
    assert os.path.samefile(path, os.path.join(PKG, "lib", "lib%s.so" % desc.link))
    macro = RS.header_macros()["FN2P_ABI_VERSION"]
    assert fn2_capi.sample_lib().fn2p_abi_version() == 0 == macro
    exported = _exported(path)
    assert exported == _declared(desc.header, "fn2p_") == sorted(fn2_capi.SAMPLE_EXPORTS) == NAMES
    assert _needed(path) == []
    # no released library, the debug twin included, exports a preview name
    for name in build.LIBRARIES:
        stem = name.upper() + "_" if name else ""
        assert not any(n.startswith("fn2p_") for n in getattr(fn2_capi, stem + "EXPORTS")), name
        assert not any(n.startswith("fn2p_") for n in _exported(getattr(fn2_capi, stem + "LIB_PATH"))), name
    assert not any(n.startswith("fn2p_") for n in fn2_capi.DEBUG_EXPORTS)


def test_module_links_exactly_its_library():
    assert _needed(os.path.join(PKG, "corr_sample_cuda" + sysconfig.get_config_var("EXT_SUFFIX"))) == ["libflownet2_hip_sample.so"]
    text = open(os.path.join(PKG, "csrc", "binding", "corr_sample_cuda.cpp")).read()
    assert "STATUS_SAMPLE" in text and "fn2_strerror(" not in text
    for lib in build.LIBRARIES.values():        # STATUS_SAMPLE is the new module's alone
        for module in lib.modules:
            assert "STATUS_SAMPLE" not in open(os.path.join(PKG, "csrc", "binding", module + ".cpp")).read(), module


def test_header_compiles_after_the_released_headers(tmp_path):
    # all seven in their documented order, each one alone in front of it, and the preview header by itself
    for i, incs in enumerate([RELEASED_HEADERS] + [[h] for h in RELEASED_HEADERS] + [[]]):
        src = tmp_path / f"hdr{i}.c"
        src.write_text("".join(f'#include "{h}"\n' for h in list(incs) + ["preview/flownet2_hip_sample.h"]) +
                       "int codes[FN2_OK - FN2_EUNSUPPORTED + FN2_BF16 + FN2P_MAX_LEVELS + FN2P_MAX_RADIUS - FN2P_BOUND_LOG2 + FN2P_ABI_VERSION];\n")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ rejections
def test_rejected_calls_return_codes_without_gpu():
    """Every call returns in front of a launch, in the header's order: there is no GPU here, and the pointers are host memory."""
    lib = fn2_capi.sample_lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 2)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*[x.value for x in v])

    def fwd(levels, H2, W2, L, co, out, B, H, W, r):
        return lib.fn2p_corr_sample_forward(levels, H2, W2, L, co, out, B, H, W, r, null)

    def bwd(levels, H2, W2, L, co, go, B, H, W, r):
        return lib.fn2p_corr_sample_backward(H2, W2, L, co, go, levels, B, H, W, r, null)

    h2, w2, good = ints(4, 2), ints(8, 4), ptrs(p, p)
    for call in (fwd, bwd):
        # 1. parameters and sizes, whatever else is wrong
        for L in (0, -1, 9):
            assert call(None, None, None, L, null, null, 1, 8, 16, 4) == EINVAL, L
        for r in (-1, 9, 100):
            assert call(None, None, None, 2, null, null, 1, 8, 16, r) == EINVAL, r
        for B, H, W in ((-1, 8, 16), (1, 0, 16), (1, 8, 0), (1, -8, 16)):
            assert call(None, None, None, 2, null, null, B, H, W, 4) == EINVAL, (B, H, W)
        for bad in (ints(4, 0), ints(-4, 2)):
            assert call(None, bad, w2, 2, null, null, 1, 8, 16, 4) == EINVAL
            assert call(None, h2, bad, 2, null, null, 1, 65536, 65536, 4) == EINVAL       # sizes before the limits
        # 2. limits: B H W >= 2^31, a slice of 2^31 cells, more than 2^48 cells in a level
        assert call(None, None, None, 2, null, null, 1, 65536, 32768, 4) == EUNSUPPORTED
        assert call(None, None, None, 2, null, null, 4, 32768, 16384, 4) == EUNSUPPORTED
        assert call(None, ints(4, 65536), ints(8, 32768), 2, null, null, 1, 8, 16, 4) == EUNSUPPORTED
        assert call(None, ints(4, 16384), ints(8, 16384), 2, null, null, 1, 1024, 1025, 4) == EUNSUPPORTED   # (2^20 + 2^10) 2^28 cells
        assert call(None, ints(4, 16384), ints(8, 16384), 2, null, null, 1, 1024, 1024, 4) == EINVAL         # 2^48 itself passes, to check 4
        assert call(None, h2, w2, 2, null, null, 0, 65536, 32768, 4) == EUNSUPPORTED                         # limits before the empty batch
        # 3. the empty batch: nothing to do, whatever the pointers
        assert call(None, None, None, 2, null, null, 0, 8, 16, 4) == OK
        assert call(ptrs(mis, null), h2, w2, 2, mis, null, 0, 8, 16, 4) == OK
        # 4. NULL arrays and pointers, also next to a misaligned one: NULL is reported first
        assert call(None, h2, w2, 2, p, mis, 1, 8, 16, 4) == EINVAL
        assert call(good, None, w2, 2, p, mis, 1, 8, 16, 4) == EINVAL
        assert call(good, h2, None, 2, p, mis, 1, 8, 16, 4) == EINVAL
        assert call(good, h2, w2, 2, null, mis, 1, 8, 16, 4) == EINVAL
        assert call(good, h2, w2, 2, mis, null, 1, 8, 16, 4) == EINVAL
        assert call(ptrs(mis, null), h2, w2, 2, p, p, 1, 8, 16, 4) == EINVAL
        assert call(ptrs(null, p), h2, w2, 2, p, p, 1, 8, 16, 4) == EINVAL
        # 5. alignment to 4 bytes
        assert call(good, h2, w2, 2, mis, p, 1, 8, 16, 4) == EALIGN
        assert call(good, h2, w2, 2, p, mis, 1, 8, 16, 4) == EALIGN
        assert call(ptrs(p, mis), h2, w2, 2, p, p, 1, 8, 16, 4) == EALIGN
        assert call(ptrs(mis, p), h2, w2, 2, p, p, 1, 8, 16, 4) == EALIGN


STATUS_PROGRAM = """
#include <cstdio>
#include "binding_status.h"
int main()
{
    const int codes[] = {-1, -2, -3, -4, 7, -9};
    for (int rc : codes) std::puts(fn2b::status_message(fn2b::STATUS_SAMPLE, "op", rc).c_str());
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
        "op: HIP call failed: flownet2_hip_sample: invalid shape or parameter (1 .. 8 levels, radius 0 .. 8) (code -1)",
        "op: HIP call failed: flownet2_hip_sample: unknown error (code -2)",
        "op: HIP call failed: flownet2_hip_sample: pointer not aligned to its element size (code -3)",
        "op: HIP call failed: flownet2_hip_sample: unsupported size (2^31 query pixels or more, a slice of 2^31 cells or more, or a level beyond 2^48 cells)"
        " (code -4)",
        "op: HIP call failed: flownet2_hip_sample: hipError_t from the launch (code 7)",
        "op: HIP call failed: flownet2_hip_sample: unknown error (code -9)"]


def test_cpu_tensors_are_refused():
    import corr_sample_cuda
    from networks.correlation_package import CorrBlock, corr_sample
    pyr, co = [torch.zeros(8, 1, 2, 4), torch.zeros(8, 1, 1, 2)], torch.zeros(1, 2, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_sample_cuda.forward_alloc(pyr, co, 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_sample_cuda.backward_alloc(pyr, co, torch.zeros(1, 50, 2, 4), 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        corr_sample(pyr, co, 2)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        CorrBlock(torch.zeros(1, 4, 2, 4), torch.zeros(1, 4, 2, 4), num_levels=2, radius=2)(co)
    with pytest.raises(RuntimeError, match="detach"):   # before anything else: a silent None would train wrongly
        corr_sample(pyr, co.clone().requires_grad_(True), 2)


# ------------------------------------------------------------------ the reference
def test_header_macros():
    assert RS.header_macros() == {"FN2P_ABI_VERSION": 0, "FN2P_MAX_LEVELS": 8, "FN2P_MAX_RADIUS": 8, "FN2P_BOUND_LOG2": -21,
                                  "FN2P_TILE_FORWARD": 32, "FN2P_TILE_BACKWARD": 16}
    assert float(RS.bound(1.0)) == 2.0 ** -21 + 8 * 2.0 ** -149


def _pyramid64(f1, f2, L):
    B, C, H, W = f1.shape
    corr = torch.matmul(f1.reshape(B, C, H * W).transpose(1, 2), f2.reshape(B, C, -1)) * float(C) ** -0.5
    pyr = [corr.reshape(B * H * W, 1, *f2.shape[2:])]
    for _ in range(L - 1):
        pyr.append(torch.nn.functional.avg_pool2d(pyr[-1], 2, stride=2))
    return pyr


@pytest.mark.parametrize("geo", [(8, 9, 3, 2), (4, 7, 2, 1), (9, 11, 3, 3), (4, 4, 1, 0)], ids=lambda g: "%dx%d-L%d-r%d" % g)
def test_reference_against_rafts_composition(geo):
    """Values and both feature-map gradients to 1e-12 relative, in float64, level sizes >= 2; coordinates at non-negative
    positions or below -1, where fl32(c - floor(c)) is exact (the header)."""
    H, W, L, r = geo
    B, C = 2, 3
    rng = np.random.default_rng(H + r)
    f1 = torch.from_numpy(rng.standard_normal((B, C, H, W))).requires_grad_(True)
    f2 = torch.from_numpy(rng.standard_normal((B, C, H, W))).requires_grad_(True)
    c = rng.uniform(-r - 2, max(H, W) + r + 2, (B, 2, H, W))
    c = np.where(c < 0, c - 2.0 ** (L - 1), c).astype(np.float32)           # c 2^-l <= -1 at every level
    go = rng.standard_normal((B, L * (2 * r + 1) ** 2, H, W))
    want = RL.compose(f1, f2, torch.from_numpy(c).double(), r, float(C) ** -0.5, num_levels=L)
    w1, w2 = torch.autograd.grad(want, (f1, f2), torch.from_numpy(go))
    pyr = [t.detach().requires_grad_(True) for t in _pyramid64(f1.detach(), f2.detach(), L)]
    got, S = RS.forward([t.detach().numpy() for t in pyr], c, r)
    scale = float(np.abs(want.detach().numpy()).max())
    assert scale > 0.1 and np.abs(got - want.detach().numpy()).max() <= 1e-12 * scale
    assert (S >= np.abs(got) - 1e-15).all()
    # the gradients of the levels, pushed through the pooling and the matmul by autograd
    ref = RS.backward([tuple(t.shape[2:]) for t in pyr], c, go, r)
    rebuilt = _pyramid64(f1, f2, L)
    g1, g2 = torch.autograd.grad(rebuilt, (f1, f2), [torch.from_numpy(g).reshape(t.shape) for (g, _, _), t in zip(ref, rebuilt)])
    for g, w in ((g1, w1), (g2, w2)):
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())
    for (g, Sg, n), t in zip(ref, pyr):
        assert (g[n == 0] == 0).all() and (Sg[n == 0] == 0).all() and 1 <= int(n.max()) <= 4


def test_channel_and_level_order():
    """A one-hot level: level 1's only non-zero cell of pixel p's slice is (y, x) = (2, 3); integer coordinates (6, 4) / 2 = (3, 2)
    put it in the window's centre, channel D^2 + r D + r; coordinates (4, 4) see it at i - r = +1, j - r = 0."""
    r, L, H, W = 2, 3, 1, 2
    D = 2 * r + 1
    levels = [np.zeros((H * W, 8 >> l, 8 >> l)) for l in range(L)]
    levels[1][:, 2, 3] = 1.0
    co = np.array([[[[6.0, 4.0]], [[4.0, 4.0]]]], dtype=np.float32)          # pixel 0 at (x, y) = (6, 4), pixel 1 at (4, 4)
    out, _ = RS.forward(levels, co, r)
    assert out.shape == (1, L * D * D, H, W)
    assert out[0, :, 0, 0].nonzero()[0].tolist() == [D * D + r * D + r] and out[0, D * D + r * D + r, 0, 0] == 1.0
    assert out[0, :, 0, 1].nonzero()[0].tolist() == [D * D + (r + 1) * D + r]
    co[0, :, 0, 1] = (6.0, 2.0)                                               # (3, 1) at level 1: i - r = 0, j - r = +1
    out, _ = RS.forward(levels, co, r)
    assert out[0, :, 0, 1].nonzero()[0].tolist() == [D * D + r * D + r + 1]
    # the backward sends channel D^2 + r D + r of pixel 0 back to that cell, and nothing anywhere else
    go = np.zeros_like(out)
    go[0, D * D + r * D + r, 0, 0] = 1.0
    ref = RS.backward([t.shape[1:] for t in levels], co, go, r)
    assert ref[1][0][0, 2, 3] == 1.0 and sum(float(np.abs(g).sum()) for g, _, _ in ref) == 1.0


# ------------------------------------------------------------------ torch.compile and the operators
def _compile(fn, **kw):
    import torch._dynamo
    torch._dynamo.reset()
    return torch.compile(fn, backend="aot_eager", fullgraph=True, **kw)


def _t(*shape, dtype=torch.float32, grad=False):
    return torch.empty(*shape, dtype=dtype, device=META, requires_grad=grad)


def _block(fmap1, fmap2, coords):
    from networks.correlation_package import CorrBlock
    return CorrBlock(fmap1, fmap2, num_levels=3, radius=2)(coords)


def test_corr_block_traces_forward_and_backward():
    import torch._dynamo
    a, b, c = _t(2, 8, 9, 11, grad=True), _t(2, 8, 9, 11, grad=True), _t(2, 2, 9, 11)
    out = _compile(_block)(a, b, c)
    assert tuple(out.shape) == (2, 75, 9, 11) and out.dtype == torch.float32 and out.requires_grad and out.is_contiguous()
    g1, g2 = torch.autograd.grad(out.sum(), (a, b))
    assert g1.shape == a.shape and g2.shape == b.shape
    torch._dynamo.reset()
    rep = torch._dynamo.explain(_block)(a, b, c)
    assert rep.graph_break_count == 0 and rep.graph_count == 1, rep.break_reasons
    out = _compile(_block)(a.half(), b.half(), c.double())         # RAFT's .float() on the maps and the coordinates
    assert out.dtype == torch.float32


def test_corr_block_dynamic_shapes_do_not_recompile():
    import torch._dynamo
    from torch._dynamo.testing import CompileCounterWithBackend
    torch._dynamo.reset()
    counter = CompileCounterWithBackend("aot_eager")
    fn = torch.compile(_block, backend=counter, fullgraph=True, dynamic=True)
    outs, frames = [], []
    # (avg_pool2d's own meta function guards on the parity of its sizes: the two shapes share it at both pooled levels)
    for H, W in ((9, 11), (13, 19)):
        a, b = _t(2, 8, H, W, grad=True), _t(2, 8, H, W, grad=True)
        out = fn(a, b, _t(2, 2, H, W))
        torch.autograd.grad(out.sum(), (a, b))
        outs.append(tuple(out.shape))
        frames.append(counter.frame_count)
    assert frames[0] >= 1 and frames[1] == frames[0], frames
    assert outs == [(2, 75, 9, 11), (2, 75, 13, 19)]


def test_mini_raft_with_corr_block_traces():
    import torch._dynamo

    import compile_cases as CC
    import pipelines_ref as P
    from networks.correlation_package import CorrBlock
    layers = types.SimpleNamespace(**{**vars(P.hip_layers()), "corr_block": lambda f1, f2, L, r: CorrBlock(f1, f2, num_levels=L, radius=r)})
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


def test_opcheck_schema_and_fake():
    import fn2_ops
    import networks.correlation_package.corr_block  # noqa: F401
    pyr = [_t(198, 1, 9, 11, grad=True), _t(198, 1, 4, 5, grad=True)]
    co = _t(2, 2, 9, 11)
    for op, args in ((torch.ops.fn2.corr_sample, (pyr, co, 2)), (torch.ops.fn2.corr_sample_backward, (pyr, co, _t(2, 50, 9, 11), 2))):
        res = torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
        assert set(res.values()) == {"SUCCESS"}, res
    assert tuple(torch.ops.fn2.corr_sample(pyr, co, 2).shape) == (2, 50, 9, 11)
    assert [tuple(g.shape) for g in torch.ops.fn2.corr_sample_backward(pyr, co, _t(2, 50, 9, 11), 2)] == [(198, 1, 9, 11), (198, 1, 4, 5)]
    # preview operators stay out of the released listing
    assert fn2_ops.names(preview=True) == ["fn2::corr_sample", "fn2::corr_sample_backward"]
    assert not any("corr_sample" in n for n in fn2_ops.names())


def test_backward_operator_is_not_differentiable_twice():
    import networks.correlation_package.corr_block  # noqa: F401
    pyr, go = [_t(198, 1, 9, 11)], _t(2, 25, 9, 11, grad=True)
    g, = torch.ops.fn2.corr_sample_backward(pyr, _t(2, 2, 9, 11), go, 2)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="not differentiable a second time"):
        g.sum().backward()


def _refusals():
    from networks.correlation_package import CorrSample, corr_sample
    pyr, co = [_t(198, 1, 9, 11, grad=True), _t(198, 1, 4, 5)], _t(2, 2, 9, 11)
    return {
        "radius": (CorrSample(9), (pyr, co), "radius 9 outside"),
        "half pyramid": (CorrSample(3), ([t.half() for t in pyr], co), "float32 tensors expected"),
        "coords grad": (CorrSample(3), (pyr, _t(2, 2, 9, 11, grad=True)), "coords requires grad"),
        "coords shape": (CorrSample(3), (pyr, _t(2, 2, 9, 12)), "a pyramid level has shape"),
        "no levels": (lambda c: corr_sample([], c, 3), (co,), "0 levels"),
    }


@pytest.mark.parametrize("which", ["radius", "half pyramid", "coords grad", "coords shape", "no levels"])
def test_refused_at_trace_time(which):
    fn, args, match = _refusals()[which]
    with pytest.raises(Exception, match=match):
        _compile(fn)(*args)
