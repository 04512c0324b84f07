"""CPU checks of tests/lowp_ref.py, the float64 references and rounding brackets of the half / bfloat16 contract tests
(tests/test_gpu_lowp_contract.py): the references against the oracle, the bracket on hand-made rounding cases, and the reason
the contract tests exist -- a kernel that rounds every product to bf16 passes the older global bound and fails the bracket."""
import numpy as np
import pytest
import torch

import lowp_ref as L

BF, HF = torch.bfloat16, torch.float16
# every parameter set of the contract tests: FlowNetC's, and the general kernel's k = 3 / stride1 = 2 ones
PARAMS = [L.CORR, (3, 3, 4, 2, 2), (3, 3, 4, 1, 2), (2, 1, 4, 2, 1)]


@pytest.mark.parametrize("params", PARAMS)
def test_corr_fwd64_matches_oracle(oracle, params):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((2, 5, 9, 12)).astype(np.float32)
    b = rng.standard_normal((2, 5, 9, 12)).astype(np.float32)
    ref = oracle.corr_fwd(a, b, *params)
    got = L.corr_fwd64(torch.from_numpy(a), torch.from_numpy(b), *params).numpy()
    absr = L.corr_fwd64(torch.from_numpy(np.abs(a)), torch.from_numpy(np.abs(b)), *params).numpy()
    assert got.shape == ref.shape
    # the oracle sums in fp32: within its own rounding of the |terms|
    assert (np.abs(got - ref) <= 2.0 ** -20 * absr + 1e-30).all(), float(np.abs(got - ref).max())
    assert (absr > 0).any() and (got == 0).sum() == (absr == 0).sum()


@pytest.mark.parametrize("params", [p for p in PARAMS if p[3] == 1])
def test_corr_bwd64_matches_oracle(oracle, params):
    rng = np.random.default_rng(4)
    a = rng.standard_normal((2, 4, 10, 13)).astype(np.float32)
    b = rng.standard_normal((2, 4, 10, 13)).astype(np.float32)
    nOut, oH, oW = L.out_shape(10, 13, *params)
    go = rng.standard_normal((2, nOut, oH, oW)).astype(np.float32)
    r1, r2 = oracle.corr_bwd(a, b, go, *params)
    g1, g2 = L.corr_bwd64(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(go), *params)
    ab1, ab2 = L.corr_bwd64(*(torch.from_numpy(np.abs(t)) for t in (a, b, go)), *params)
    for got, ref, ab in ((g1, r1, ab1), (g2, r2, ab2)):
        assert (np.abs(got.numpy() - ref) <= 2.0 ** -18 * ab.numpy() + 1e-30).all(), float(np.abs(got.numpy() - ref).max())


def test_corr_bwd64_is_the_gradient_of_corr_fwd64():
    """The backward reference is the exact adjoint of the forward one (autograd through corr_fwd64), FlowNetC and k = 3."""
    g = torch.Generator().manual_seed(5)
    for params, shape in ((L.CORR, (1, 3, 6, 8)), ((3, 3, 4, 1, 2), (2, 3, 7, 9))):
        a = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
        out = L.corr_fwd64(a, b, *params)
        go = torch.randn(out.shape, generator=g, dtype=torch.float64)
        out.backward(go)
        g1, g2 = L.corr_bwd64(a.detach(), b.detach(), go, *params)
        assert torch.allclose(g1, a.grad, rtol=1e-12, atol=1e-14) and torch.allclose(g2, b.grad, rtol=1e-12, atol=1e-14)


def _br(values, delta, dtype):
    lo, hi = L.bracket(torch.tensor(values, dtype=torch.float64), delta, dtype)
    return lo.float().tolist(), hi.float().tolist()


def test_bracket_ties():
    # bf16 around 1: spacing 2^-7; 1 + 2^-8 is a tie -> even (1.0); 1 + 3*2^-8 is a tie -> even (1 + 2^-6)
    lo, hi = _br([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8], 0.0, BF)
    assert lo == hi == [1.0, 1 + 2.0 ** -6]
    # any delta moves a tie's bracket to both neighbours
    lo, hi = _br([1 + 2.0 ** -8], 2.0 ** -30, BF)
    assert lo == [1.0] and hi == [1 + 2.0 ** -7]
    # half around 1: spacing 2^-10
    lo, hi = _br([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11)], 0.0, HF)
    assert lo == hi == [1.0, 1 + 2.0 ** -9, -1.0]
    lo, hi = _br([1 + 2.0 ** -11], 2.0 ** -40, HF)
    assert lo == [1.0] and hi == [1 + 2.0 ** -10]


def test_bracket_half_overflow_threshold():
    lo, hi = _br([65504.0, 65519.0, 65520.0, -65520.0, 1e6], 0.0, HF)
    assert lo == hi == [65504.0, 65504.0, float("inf"), -float("inf"), float("inf")]
    lo, hi = _br([65519.0], 2.0, HF)     # the bracket straddles the threshold: either is allowed
    assert lo == [65504.0] and hi == [float("inf")]
    lo, hi = _br([3.0e38], 0.0, BF)      # bf16's own threshold (fp32's range)
    assert lo == hi == [float(torch.tensor(3.0e38).to(BF))]
    lo, hi = _br([3.5e38], 0.0, BF)      # past fp32: infinite before the 16-bit rounding
    assert lo == hi == [float("inf")]


def test_bracket_half_subnormals():
    s = 2.0 ** -24                       # smallest half subnormal
    lo, hi = _br([s, 3 * s, 2.5 * s, 0.5 * s, 1.5 * s, 0.25 * s], 0.0, HF)
    assert lo == hi == [s, 3 * s, 2 * s, 0.0, 2 * s, 0.0]
    lo, hi = _br([2.5 * s], 2.0 ** -40, HF)
    assert lo == [2 * s] and hi == [3 * s]


def test_bracket_exact_ref_delta_zero():
    """delta = 0 and a float32-exact ref: lo == hi == RNE(ref), for both types, against torch's own float32 -> 16-bit rounding."""
    g = torch.Generator().manual_seed(9)
    x32 = torch.cat([torch.randn(20000, generator=g) * 2.0 ** torch.randint(-30, 16, (20000,), generator=g).float(),
                     torch.tensor([0.0, -0.0, 2.0 ** -130, 1e-45])])
    for dt in (BF, HF):
        lo, hi = L.bracket(x32.double(), 0.0, dt)
        want = x32.to(dt)
        assert torch.equal(lo.view(torch.int16), hi.view(torch.int16)) or torch.equal(lo, hi)
        assert torch.equal(lo.float(), want.float()) and torch.equal(hi.float(), want.float())


def test_bracket_no_double_rounding():
    """A float64 value just above a bf16 tie: float64 -> float32 would land on the tie and round to even (down); the bracket
    rounds up to float32 first and keeps the upper neighbour reachable."""
    x = 1 + 2.0 ** -8 + 2.0 ** -40
    assert float(torch.tensor(x, dtype=torch.float64).to(BF)) == 1.0          # torch's two roundings
    lo, hi = _br([x], 0.0, BF)
    assert lo == [1.0] and hi == [1 + 2.0 ** -7]


def test_fused_leaky_posts():
    """The two fused LeakyReLU sequences: slope on fp32 then one rounding (matrix kernels), rounding, slope, rounding (general)."""
    x = torch.tensor([-(1 + 2.0 ** -9 + 2.0 ** -12)], dtype=torch.float64)   # not a bf16 value
    lm = L.bracket(x, 0.0, BF, post=L.leaky_matrix(0.1, BF))
    lg = L.bracket(x, 0.0, BF, post=L.leaky_general(0.1, BF))
    s = torch.tensor(0.1, dtype=torch.float32)
    assert float(lm[0]) == float((x.float() * s).to(BF))
    assert float(lg[0]) == float((x.float().to(BF).float() * s).to(BF))


# ------------------------------------------------------------------ the mutation check
def _bf16_round(t):
    return t.float().to(BF).double()


@pytest.mark.parametrize("case", [(2, 128, 46, 56), (1, 384, 2, 56)])
def test_bracket_rejects_product_rounding_kernel(case):
    """A kernel that rounds every product to bf16 before summing (simulated here in float64 on the contract tests' family-1
    inputs, result rounded once): the older global bound 2^-8 max|ref| accepts it, the per-element bracket rejects it.  The
    bracket also rejects a 1/C rounded to bf16 (C = 384: not a power of two), which the global bound only just catches at the
    largest output, where that relative error of 2^-9 is largest."""
    B, C, H, W = case
    a, b = L.family_inputs(1, case, BF, seed=sum(case))                    # test_gpu_lowp_contract.py's seed
    ref = L.corr_fwd64(a, b, *L.CORR)
    absr = L.corr_fwd64(a.abs(), b.abs(), *L.CORR)
    lo, hi = L.bracket(ref, L.delta_fwd(ref, absr, C), BF)
    correct = ref.float().to(BF)                                           # an exact kernel: inside
    assert not L.outside(correct, lo, hi).any()
    mut = L.corr_fwd64(a, b, *L.CORR, prod=lambda x, y: _bf16_round(x * y)).float().to(BF)
    glob = 2.0 ** -8 * float(ref.abs().max())
    assert float((mut.double() - ref).abs().max()) <= glob                 # the existing bound accepts it ...
    live = int((absr > 0).sum())                                           # outputs that are not all padding
    n_out = int(L.outside(mut, lo, hi).sum())
    assert n_out > 0.01 * live, (n_out, live)                              # ... the bracket does not
    if C & (C - 1):
        rc = float(torch.tensor(1.0 / C).to(BF))
        mut_c = (ref * C * rc).float().to(BF)
        assert int(L.outside(mut_c, lo, hi).sum()) > 0.01 * live
