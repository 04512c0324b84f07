"""The correlation backward kernels walk only the neighbour row blocks that meet the image (csrc/corr_params.h: bwd_u_range).  The
shapes below hit every path that adds, at the smallest sizes that still have it: a single real block, leading and trailing empty blocks
in one task, tasks of different first blocks and odd step counts following each other on one workgroup (the cross-task prefetch and
the hand-over of the staging waves' register sets), and the benchmark's row geometry.  Bars: those of
test_gpu_parity.py::test_correlation_f16x2_backward_vs_oracle (fp32) and of the half / bfloat16 backward tests."""
import numpy as np
import pytest
import torch

from conftest import max_abs
from test_bwd_u_range_host import steps_per_workgroup

pytestmark = pytest.mark.gpu

TOL = 1e-4
CORR = (20, 1, 20, 1, 2)
CASES = [
    (1, 64, 2, 8),       # one real block of six
    (1, 64, 10, 16),     # HL = 5: ragged last row group, leading and trailing empties in one task
    (1, 64, 24, 8),      # four real blocks in every task; empties on both sides of the middle row group
    (1, 64, 48, 8),      # the benchmark's six row groups: 4, 5, 6, 6, 5, 4 blocks
    (22, 64, 48, 8),     # 528 tasks on 256 workgroups: different first blocks and odd counts follow each other on a workgroup
    (3, 256, 48, 64),    # 288 tasks: four channel groups, multi-task workgroups at the benchmark's geometry
]
_cache = {}


def _case(oracle, case):
    """Seeded fp32 inputs of a shape and the oracle's gradients for them: computed once, shared, never modified."""
    if case not in _cache:
        B, C, H, W = case
        rng = np.random.default_rng(B * 1000 + C * 7 + H + W + 11)
        a = rng.standard_normal((B, C, H, W)).astype(np.float32)
        b = rng.standard_normal((B, C, H, W)).astype(np.float32)
        go = rng.standard_normal((B, 441, H, W)).astype(np.float32)
        _cache[case] = (a, b, go) + tuple(oracle.corr_bwd(a, b, go, *CORR))
    return _cache[case]


def _dev(dev, *arrays):
    return [torch.from_numpy(x).to(dev) for x in arrays]


@pytest.mark.parametrize("case", CASES)
def test_f16x2_backward_real_row_blocks_vs_oracle(dev, oracle, case):
    import fn2_capi
    B, C, H, W = case
    a, b, go, r1, r2 = _case(oracle, case)
    ad, bd, gd = _dev(dev, a, b, go)
    scale = max(1.0, float(np.abs(r1).max()))
    res = {}
    for algo in (fn2_capi.FN2_CORR_MFMA_F16X2, fn2_capi.FN2_CORR_AUTO):
        g1 = torch.full((B, C, H, W), float("nan"), device=dev)
        g2 = torch.full((B, C, H, W), float("nan"), device=dev)
        fn2_capi.correlation_backward(ad, bd, gd, *CORR, algo=algo, out=(g1, g2))
        n1, n2 = g1.cpu().numpy(), g2.cpu().numpy()
        assert np.isfinite(n1).all() and np.isfinite(n2).all(), "unwritten gradient elements"
        e1, e2 = max_abs(n1, r1), max_abs(n2, r2)
        print(case, algo, "max abs error", e1, e2, "scale", scale)
        assert e1 <= TOL and e2 <= TOL, (algo, e1, e2)
        assert e1 <= 5e-6 * scale and e2 <= 5e-6 * scale, (algo, e1, e2)
        res[algo] = (g1, g2)
    assert torch.equal(res[fn2_capi.FN2_CORR_AUTO][0], res[fn2_capi.FN2_CORR_MFMA_F16X2][0])
    assert torch.equal(res[fn2_capi.FN2_CORR_AUTO][1], res[fn2_capi.FN2_CORR_MFMA_F16X2][1])


@pytest.mark.parametrize("case", [(1, 64, 28, 72), (2, 64, 8, 96)])
def test_wide_backward_real_steps_vs_oracle(dev, oracle, case):
    """Maps wider than 64 px (the column-window kernel: its (pass, u) step list holds the real row blocks only).  28 x 72: row groups
    of 4, 4, 4, 3 real blocks; window 0 runs two passes, window 1 one -- 3 steps in the last row group: an odd count and the hand-over
    of the register sets.  8 x 96: two real blocks of six in each pass.  Bar: test_correlation_f16x2_backward_wide_vs_oracle's."""
    import fn2_capi
    B, C, H, W = case
    a, b, go, r1, r2 = _case(oracle, case)
    ad, bd, gd = _dev(dev, a, b, go)
    scale = max(1.0, float(np.abs(r1).max()))
    res = {}
    for algo in (fn2_capi.FN2_CORR_MFMA_F16X2, fn2_capi.FN2_CORR_AUTO):
        g1 = torch.full((B, C, H, W), float("nan"), device=dev)
        g2 = torch.full((B, C, H, W), float("nan"), device=dev)
        fn2_capi.correlation_backward(ad, bd, gd, *CORR, algo=algo, out=(g1, g2))
        n1, n2 = g1.cpu().numpy(), g2.cpu().numpy()
        assert np.isfinite(n1).all() and np.isfinite(n2).all(), "unwritten gradient elements"
        e1, e2 = max_abs(n1, r1), max_abs(n2, r2)
        print(case, algo, "max abs error", e1, e2, "scale", scale)
        assert e1 <= 5e-6 * scale and e2 <= 5e-6 * scale, (algo, e1, e2)
        res[algo] = (g1, g2)
    assert torch.equal(res[fn2_capi.FN2_CORR_AUTO][0], res[fn2_capi.FN2_CORR_MFMA_F16X2][0])
    assert torch.equal(res[fn2_capi.FN2_CORR_AUTO][1], res[fn2_capi.FN2_CORR_MFMA_F16X2][1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", CASES[:5])
def test_16bit_backward_row_blocks_vs_oracle(dev, oracle, case, dtype):
    """The half / bfloat16 backward kernel on the same row geometries, against the oracle on the rounded inputs.  Bars: half as
    test_correlation_half_backward_matrix_kernel (one rounding of each result to half), bfloat16 as test_bf16_correlation_backward."""
    import fn2_capi
    B, C, H, W = case
    rng = np.random.default_rng(B * 1000 + C + H + W + 13)
    a, b, go = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dtype) for s in ((B, C, H, W), (B, C, H, W), (B, 441, H, W)))
    r1, r2 = oracle.corr_bwd(a.float().numpy(), b.float().numpy(), go.float().numpy(), *CORR)
    g1 = torch.full((B, C, H, W), float("nan"), dtype=dtype, device=dev)
    g2 = torch.full((B, C, H, W), float("nan"), dtype=dtype, device=dev)
    fn2_capi.correlation_backward(a.to(dev), b.to(dev), go.to(dev), *CORR, out=(g1, g2))
    for got, ref in ((g1, r1), (g2, r2)):
        n = got.float().cpu().numpy()
        assert np.isfinite(n).all(), "unwritten gradient elements"
        print(case, dtype, "max abs error", float(np.abs(n - ref).max()), "scale", float(np.abs(ref).max()))
        if dtype == torch.float16:
            assert (np.abs(n - ref) <= 2.0 ** -11 * np.abs(ref) + 2e-6 * np.abs(ref).max() + 1e-7).all(), float(np.abs(n - ref).max())
        else:
            assert max_abs(n, ref) <= 2.0 ** -8 * float(np.abs(ref).max()) + 1e-6


def test_fused_backward_equals_unfused_on_multi_task_workgroups(dev):
    """fn2_correlation_backward_fused runs the same kernel on the masked gradient: bit-identical at the shape whose workgroups run
    tasks of different first blocks and odd step counts."""
    import fn2_capi
    B, C, H, W, Cr = 22, 64, 48, 8, 8
    g = torch.Generator().manual_seed(2248)
    a = torch.randn(B, C, H, W, generator=g).to(dev)
    b = torch.randn(B, C, H, W, generator=g).to(dev)
    buf = torch.randn(B, Cr + 441, H, W, generator=g).to(dev)          # stands for the forward's concat buffer: only its sign is used
    gbuf = torch.randn(B, Cr + 441, H, W, generator=g).to(dev)
    f1, f2 = fn2_capi.correlation_backward_fused(a, b, buf, gbuf, Cr, 0.1, *CORR)
    out, gs = buf[:, Cr:], gbuf[:, Cr:]
    masked = torch.where(out > 0, gs, gs * 0.1).contiguous()
    u1, u2 = fn2_capi.correlation_backward(a, b, masked, *CORR)
    assert torch.equal(f1, u1) and torch.equal(f2, u2)


def test_executed_steps_match_the_host_model(dev, oracle):
    """The profiling instantiation (debug library, variant 6064: correct results plus stamps) reports the row-block steps every
    workgroup executed in the matrix wave's slot 1 of its stamp record: they equal the host model's, workgroup by workgroup."""
    import fn2_capi
    case = (22, 64, 48, 8)
    B, C, H, W = case
    a, b, go, r1, r2 = _case(oracle, case)
    ad, bd, gd = _dev(dev, a, b, go)
    want, ntasks = steps_per_workgroup(B, C, H, W)
    assert ntasks == 528 and len(want) == 256 and len(set(want)) > 1
    stamps = torch.zeros(256 * 2 * 16, dtype=torch.int64, device=dev)
    dbg = fn2_capi.debug_lib()
    dbg.fn2_debug_set_buffer(fn2_capi._p(stamps))
    try:
        g1, g2 = fn2_capi.correlation_backward(ad, bd, gd, *CORR, algo=6064)
        torch.cuda.synchronize()
    finally:
        dbg.fn2_debug_set_buffer(None)
    got = stamps.cpu().view(256, 2, 16)[:, 1, 1].tolist()
    assert got == want, [(w, g, e) for w, (g, e) in enumerate(zip(got, want)) if g != e][:8]
    assert sum(got) < 6 * ntasks                                        # fewer than the full loop's
    scale = max(1.0, float(np.abs(r1).max()))
    assert max_abs(g1.cpu().numpy(), r1) <= 5e-6 * scale and max_abs(g2.cpu().numpy(), r2) <= 5e-6 * scale
