"""The parameter-general correlation kernels off FlowNetC's configuration, on the CPU (no GPU): tests/corr_general_ref.py's numpy
restatement of corr_fwd_direct / corr_bwd_direct (csrc/correlation_direct.hip) meets the per-element bounds of
tests/corr_contract_ref.py on every case of GRID and every finite input family, so a GPU failure of
tests/test_gpu_corr_general.py is the kernel's and not the bound's; the same model with one indexing mistake each (MUTATIONS)
leaves the bounds on at least one grid case, so the grid tells those kernels from the right one; and the oracle, an independent
restatement of the reference's kernels, lies in the fp32 bracket of lowp_ref's float64 references on the whole grid.

Every test prints what it measured: the model's worst err / delta, and per mutation the grid cases that catch it."""
import numpy as np
import pytest
import torch

import corr_contract_ref as R
import corr_general_ref as G
import lowp_ref as L

FAMILIES = (1, 2, 3, 4, 5, 6, 7, 8)            # the finite families of corr_contract_ref.family_inputs that take any shape
BWD_GRID = [c for c in G.GRID if c[0][3] == 1]
F32, F64 = torch.float32, torch.float64


def _inputs(case, fam, double=False):
    params, shape = case
    a, b = R.family_inputs(fam, shape, seed=sum(shape) + sum(params))
    return (a.double(), b.double()) if double else (a, b)


def _gout(case, kind, seed, double=False):
    params, (B, C, H, W) = case
    g = R.grad_output(kind, (B,) + L.out_shape(H, W, *params), seed)
    return g.double() if double else g


def _fwd_refs(a, b, params):
    return L.corr_fwd64(a, b, *params), L.corr_fwd64(a.abs(), b.abs(), *params)


def _bwd_refs(a, b, go, params):
    return L.corr_bwd64(a, b, go, *params), L.corr_bwd64(a.abs(), b.abs(), go.abs(), *params)


def test_grid_is_the_documented_one():
    assert len(G.GRID) == 19 and len(set(G.GRID)) == 19
    assert {p[1] for p, _ in G.GRID} == {1, 2, 3, 5} and {p[3] for p, _ in G.GRID} == {1, 2, 3}
    assert any(p[0] < p[2] for p, _ in G.GRID) and any(p[0] > p[2] for p, _ in G.GRID) and any(p[2] == 0 for p, _ in G.GRID)
    assert any(p[1] == 1 and p[2] % p[4] for p, _ in G.GRID)
    assert {s[1] % 4 for p, s in G.GRID if p[1] > 1} == {0, 1, 2, 3}                  # every C % 4 next to k > 1
    assert any(s[2:] == (1, 1) for _, s in G.GRID) and any(s[2] == 1 and s[3] > 64 for _, s in G.GRID)
    for pad, k, md, s1, s2 in ((4, 3, 4, 1, 2), (6, 5, 6, 1, 3)):                     # the out-of-buffer regime of the header
        assert md - (md // s2) * s2 < (k - 1) // 2 and any(p == (pad, k, md, s1, s2) for p, _ in G.GRID)


def test_output_shapes_and_the_empty_output():
    """lowp_ref.out_shape is the library's shape math on every grid case; the empty output is FN2_EINVAL (code -1)."""
    import fn2_capi
    for params, (B, C, H, W) in G.GRID:
        assert fn2_capi.correlation_output_shape(H, W, *params) == L.out_shape(H, W, *params), params
    params, (B, C, H, W) = G.EMPTY
    assert 0 in L.out_shape(H, W, *params)
    assert fn2_capi.lib().fn2_correlation_output_shape(H, W, *params, None, None, None) == -1
    with pytest.raises(RuntimeError, match=r"code -1"):
        fn2_capi.correlation_output_shape(H, W, *params)


@pytest.mark.parametrize("case", G.GRID, ids=G.case_id)
def test_model_forward_meets_the_bound(case):
    params, (B, C, H, W) = case
    worst = 0.0
    for fam in FAMILIES:
        a, b = _inputs(case, fam)
        ref, absr = _fwd_refs(a, b, params)
        ok, ratio = G.inside(G.model_fwd(a.numpy(), b.numpy(), params), ref, R.delta_direct_f32(ref, absr, C, params[1]))
        assert ok, (case, fam, ratio)
        worst = max(worst, ratio)
    # double tensors: products in double, rounded to float, the float accumulator's result is exact in double
    a, b = _inputs(case, 1, double=True)
    ref, absr = _fwd_refs(a, b, params)
    out = G.model_fwd(a.numpy(), b.numpy(), params)
    assert out.dtype == np.float64 and np.array_equal(out, out.astype(np.float32).astype(np.float64))
    ok, r64 = G.inside(out.astype(np.float32), ref, R.delta_direct_f32(ref, absr, C, params[1]))
    assert ok, (case, "double", r64)
    print(f"  model forward {G.case_id(case)}: worst err/delta float {worst:.3g}, double {r64:.3g}")


@pytest.mark.parametrize("case", BWD_GRID, ids=G.case_id)
def test_model_backward_meets_the_bound(case):
    params, (B, C, H, W) = case
    n = L.n_bwd(params[2], params[4], params[1])
    worst = 0.0
    for fam in FAMILIES:
        for kind in ("normal", "window") if fam == 1 else ("normal",):
            a, b = _inputs(case, fam)
            go = _gout(case, kind, fam)
            (r1, r2), (ab1, ab2) = _bwd_refs(a, b, go, params)
            g1, g2 = G.model_bwd(a.numpy(), b.numpy(), go.numpy(), params)
            for got, r, ab, name in ((g1, r1, ab1, "grad_input1"), (g2, r2, ab2, "grad_input2")):
                ok, ratio = G.inside(got, r, R.delta_direct_bwd_f32(r, ab, n))
                assert ok, (case, fam, kind, name, ratio)
                worst = max(worst, ratio)
    a, b = _inputs(case, 1, double=True)
    go = _gout(case, "normal", 1, double=True)
    (r1, r2), (ab1, ab2) = _bwd_refs(a, b, go, params)
    g1, g2 = G.model_bwd(a.numpy(), b.numpy(), go.numpy(), params)
    w64 = 0.0
    for got, r, ab in ((g1, r1, ab1), (g2, r2, ab2)):
        ok, ratio = G.inside(got, r, R.delta_direct_bwd_f64(r, ab, n), F64)
        assert ok, (case, "double", ratio)
        w64 = max(w64, ratio)
    print(f"  model backward {G.case_id(case)}: worst err/delta float {worst:.3g}, double {w64:.3g}")


def _caught_fwd(case, mutation):
    params, (B, C, H, W) = case
    a, b = _inputs(case, 1)
    ref, absr = _fwd_refs(a, b, params)
    return not G.inside(G.model_fwd(a.numpy(), b.numpy(), params, mutation), ref, R.delta_direct_f32(ref, absr, C, params[1]))[0]


def _caught_bwd(case, mutation):
    params, (B, C, H, W) = case
    a, b = _inputs(case, 1)
    go = _gout(case, "normal", 1)
    (r1, r2), (ab1, ab2) = _bwd_refs(a, b, go, params)
    n = L.n_bwd(params[2], params[4], params[1])
    g1, g2 = G.model_bwd(a.numpy(), b.numpy(), go.numpy(), params, mutation)
    return not (G.inside(g1, r1, R.delta_direct_bwd_f32(r1, ab1, n))[0] and G.inside(g2, r2, R.delta_direct_bwd_f32(r2, ab2, n))[0])


@pytest.mark.parametrize("mutation", sorted(G.MUTATIONS))
def test_every_mutation_leaves_the_bracket_on_some_grid_case(mutation):
    """Unit-normal inputs (family 1), gradOutput 'normal'.  A mutation of the forward is looked for in the forward's bracket, one
    of the backward in either gradient's; 'nelems' and 'kr' change both kernels and must be caught in each."""
    assert mutation in G.FWD_MUTATIONS or mutation in G.BWD_MUTATIONS
    print(f"  mutation {mutation}: {G.MUTATIONS[mutation]}")
    if mutation in G.FWD_MUTATIONS:
        fwd = [G.case_id(c) for c in G.GRID if _caught_fwd(c, mutation)]
        print(f"    forward: caught by {len(fwd)} of {len(G.GRID)} grid cases: {', '.join(fwd)}")
        assert fwd, mutation
    if mutation in G.BWD_MUTATIONS:
        bwd = [G.case_id(c) for c in BWD_GRID if _caught_bwd(c, mutation)]
        print(f"    backward: caught by {len(bwd)} of {len(BWD_GRID)} grid cases: {', '.join(bwd)}")
        assert bwd, mutation
    if mutation == "kr":
        even_k = G.case_id(((4, 2, 4, 1, 3), (2, 4, 6, 8)))
        assert fwd == [even_k] and bwd == [even_k], "kr = k / 2 differs from (k - 1) / 2 on the even kernel_size alone"


@pytest.mark.parametrize("case", G.GRID, ids=G.case_id)
def test_oracle_lies_in_the_bracket_of_the_float64_reference(oracle, case):
    """The oracle (the reference's kernels in plain C: 32 strided fp32 partial sums and a tree in the forward, 32 partial sums
    added serially in the backward) against lowp_ref.corr_fwd64 / corr_bwd64: inside the fp32 bracket of a sum of that many
    terms.  This ties the float64 references to an independent restatement on every parameter set of the grid."""
    params, (B, C, H, W) = case
    k = params[1]
    worst_f = worst_b = 0.0
    for fam in (1, 2, 3, 5, 7, 8):
        a, b = _inputs(case, fam)
        ref, absr = _fwd_refs(a, b, params)
        ok, ratio = G.inside(oracle.corr_fwd(a.numpy(), b.numpy(), *params), ref, R.delta_fma_chain(ref, absr, k * k * C))
        assert ok, (case, fam, ratio)
        worst_f = max(worst_f, ratio)
        if params[3] != 1:
            continue
        go = _gout(case, "normal", fam)
        (r1, r2), (ab1, ab2) = _bwd_refs(a, b, go, params)
        n = L.n_bwd(params[2], params[4], k)
        for got, r, ab in zip(oracle.corr_bwd(a.numpy(), b.numpy(), go.numpy(), *params), (r1, r2), (ab1, ab2)):
            ok, ratio = G.inside(got, r, R.delta_direct_bwd_f32(r, ab, n))
            assert ok, (case, fam, ratio)
            worst_b = max(worst_b, ratio)
    print(f"  oracle {G.case_id(case)}: worst err/delta forward {worst_f:.3g}, backward {worst_b:.3g}")


# ------------------------------------------------------------------ the fp32 matrix kernels' launch predicates
def test_matrix_kernel_predicates_on_the_gpu_tests_shapes():
    """What tests/test_gpu_corr_general.py relies on to say which kernel it reached."""
    assert [G.mfma_nv(md) for md in (4, 6, 8, 12, 14, 16, 20)] == [2, 3, 3, 4, 5, 5, 6]
    for md in (4, 8, 12, 16, 20):
        assert G.bf16x3_fwd_accepts(64, 16, md) and G.mfma_fwd_x4(16, md)
        assert not G.bf16x3_fwd_accepts(32, 18, md) and not G.mfma_fwd_x4(18, md)                 # W % 4 != 0
        assert not G.bf16x3_fwd_accepts(64, 72, md) and G.mfma_fwd_x4(72, md) and G.mfma_x_tiles(72) == 2
    for md in (6, 14):                                                                            # an odd radius
        assert not G.bf16x3_fwd_accepts(64, 16, md) and not G.mfma_fwd_x4(16, md)
