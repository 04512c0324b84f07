"""The n_nz bounds of tests/split_terms_ref.py on the CPU, no GPU.  Per scheme -- bf16x3 forward (n = C), bf16x3 backward (n = 441),
the pyramid's level 0 and pooled levels, f16x2 forward at C = 320, f16x2 backward (n = 441):

  * the sequential-fp32 model of the scheme meets the n_nz bound, and gives +0 where n_nz = 0, on every sparse input that
    tests/test_gpu_split_terms.py runs (the worst error / bound is printed);
  * every mutant of the model -- a dropped or mis-paired partial product, a stale l image of one staging slot, a wrong carry of
    the backward's neighbour fragments -- leaves the n_nz bound, while the dense check that the suite had (family 1 of
    corr_contract_ref.family_inputs at the same shape, n = all terms) accepts it: printed as "current dense check: ACCEPT, n_nz
    bound: REJECT" and asserted for bf16x3 at n >= 32 and f16x2 at n >= 320;
  * the conditions that give the GPU inputs their power, on the inputs alone: at least half of the output elements with a term
    inside the image have 1 <= n_nz <= 4; every channel (every position of a 32-channel stage, in the first stage and a later one,
    and of a ragged last stage) is the only non-zero term of some output; in the backward the same for every displacement plane
    that has a term at all at the shapes of the cases (at (H, W) those are |dy| < H, |dx| < W: an 8-row image has no term in 14 of
    the 21 plane rows, for any input), over a case's inputs and both gradients.
"""
import pytest
import torch

import corr_contract_ref as R
import corr_pyramid_ref as RP
import lowp_ref as L
import split_terms_ref as T
import test_corr_contract_host as H
import test_gpu_f32_contract as G

CORR = L.CORR
sid = lambda s: "x".join(map(str, s))


def _verdict(name, dense_ok, nz_ok, dense_ratio, nz_ratio):
    print(f"  {name}: current dense check: {'ACCEPT' if dense_ok else 'reject'} ({dense_ratio:.3g}), "
          f"n_nz bound: {'accept' if nz_ok else 'REJECT'} ({nz_ratio:.3g} x the bound)")


# ------------------------------------------------------------------ the restated bounds and the builders
def test_restated_bounds_are_the_suites_at_full_count():
    shape = (1, 64, 6, 16)
    a, b = R.family_inputs(1, shape, seed=1)
    ref, absr, s1, s2, s3 = R.fwd_sums(a, b, CORR, wide=False)
    for C in (64, 320):
        assert torch.equal(T.delta_f16x2_fwd(ref, absr, s1, s2, s3, C, C), R.delta_f16x2_fwd(ref, absr, s1, s2, s3, C))
    go = R.grad_output("normal", (1, 441, 6, 16), 2)
    (r1, d1, n1), (r2, d2, n2) = T.bwd_f16x2(a, b, go, n=441)
    (q1, e1), (q2, e2), _ = R.bwd_deltas(a, b, go, CORR)
    assert torch.equal(d1, e1) and torch.equal(d2, e2) and torch.equal(r1, q1) and torch.equal(r2, q2)
    # dense operands: n_nz is the number of terms inside the image
    cnt1, cnt2 = L.corr_bwd64(torch.ones_like(a), torch.ones_like(a), torch.ones_like(go), *CORR)
    assert torch.equal(n1, torch.round(64 * cnt1)) and torch.equal(n2, torch.round(64 * cnt2)) and int(n1.max()) == 3 * 8
    assert torch.equal(T.nnz_fwd(a, b, CORR), torch.round(64 * L.corr_fwd64(torch.ones_like(a), torch.ones_like(b), *CORR)))
    pshape = RP.SHAPES[0]
    f1, f2 = RP.inputs(pshape, seed=3)
    levels, S0 = RP.forward(f1, f2, pshape[4])
    C = pshape[1]
    for x, y in zip(T.pyramid_bounds(levels, S0, C, torch.full_like(S0, C)), RP.bounds(levels, S0, C)):
        assert torch.equal(x, y)
    assert bool((T.nnz_pyramid(f1, f2) == C).all())
    # a count below the full one gives a smaller bound, never a larger one
    assert bool((T.delta_x3(levels[0], S0, torch.ones_like(S0), C) < R.delta_bf16x3(levels[0], S0, C)).all())


@pytest.mark.parametrize("split", ["bf16x3", "f16x2"])
def test_builders_keep_the_small_terms_large(split):
    shape = (2, 64, 6, 20)
    a, b = T.channel_sparse(shape, 0.2, 1, split)
    go = T.grad_sparse((2, 441, 6, 20), 0.01, 1, split)
    oc, _ = T.one_channel(shape, 7, 1, split)
    assert bool((oc[:, 7] != 0).all()) and int((oc != 0).sum()) == oc[:, 7].numel()
    for t, d in ((a, 0.2), (b, 0.2), (go, 0.01)):
        x = t.numpy()
        nz = x != 0
        assert 0.8 * d < nz.mean() < 1.25 * d
        assert bool((x.view("uint32")[nz] & 1).all()), "full 24-bit mantissas"
        v = x[nz]
        if split == "bf16x3":
            h, m, l = T.split3(v)
            assert bool((abs(m) >= 2.0 ** -9 * abs(v)).all()) and bool((abs(l) >= 2.0 ** -17 * abs(v)).all())
            assert bool((h.astype("float64") + m + l == v).all())
        else:
            h, l = T.split2(v)
            normal = abs(v) >= 2.0 ** -13                       # an f16-normal h at scale exponent 0 (or one up)
            step = 2.0 ** -10 * 2.0 ** torch.floor(torch.log2(torch.from_numpy(abs(v)).double())).numpy()
            assert normal.mean() > 0.99 and bool((abs(l)[normal] >= 0.25 * step[normal]).all())
    assert not torch.equal(a != 0, b != 0)


# ------------------------------------------------------------------ bf16x3 Correlation forward
def _fwd_sums(a, b, params):
    return L.corr_fwd64(a, b, *params), L.corr_fwd64(a.abs(), b.abs(), *params)


@pytest.mark.parametrize("md", T.X3_FWD_MD)
@pytest.mark.parametrize("shape", T.X3_FWD_SHAPES, ids=sid)
def test_bf16x3_forward(shape, md):
    params = T.params_md(md)
    C = shape[1]
    any_term = L.corr_fwd64(torch.ones(shape), torch.ones(shape), *params) > 0
    for name, a, b in T.x3_fwd_inputs(shape):
        ref, absr = _fwd_sums(a, b, params)
        n = T.nnz_fwd(a, b, params)
        delta = T.delta_x3(ref, absr, n, C)
        got = T.model_x3_fwd(a, b, params)
        ok, ratio = T.inside(got, ref, delta)
        print(f"  bf16x3 fwd {shape} md {md} {name}: correct model, worst error / n_nz bound {ratio:.3g}")
        assert ok and T.plus_zero_where(got, n)
        if name != "channel_sparse":
            assert int(n.max()) == 1
            continue
        # the conditions on the input
        frac = T.small_count_fraction(n, any_term)
        sole = T.sole_terms_fwd(a, b, params)
        print(f"  1 <= n_nz <= 4 on {frac:.3f} of the outputs with a term; {len(sole)} of {C} channels are some output's only term")
        assert frac >= 0.5 and sole == set(range(C))
        # the mutants, and what the dense check says about them
        da, db = R.family_inputs(1, shape, seed=sum(shape))
        dref, dabs = _fwd_sums(da, db, params)
        ddelta = R.delta_bf16x3(dref, dabs, C)
        assert T.inside(T.model_x3_fwd(da, db, params), dref, ddelta)[0]
        for mutant in T.X3_MUTANTS:
            nz_ok, nz_ratio = T.inside(T.model_x3_fwd(a, b, params, mutant), ref, delta)
            dense_ok, dense_ratio = T.inside(T.model_x3_fwd(da, db, params, mutant), dref, ddelta)
            _verdict(f"bf16x3 fwd {shape} md {md} {mutant}", dense_ok, nz_ok, dense_ratio, nz_ratio)
            assert not nz_ok and dense_ok


# ------------------------------------------------------------------ bf16x3 Correlation backward
@pytest.mark.parametrize("shape", T.X3_BWD_SHAPES, ids=sid)
def test_bf16x3_backward(shape):
    B, C, Hh, W = shape
    one = torch.ones(shape)
    any1, any2 = (t > 0 for t in L.corr_bwd64(one, one, torch.ones(T._gshape(shape)), *CORR))
    da, db = R.family_inputs(1, shape, seed=sum(shape))
    dgo = R.grad_output("normal", T._gshape(shape), sum(shape))
    dr = L.corr_bwd64(da, db, dgo, *CORR)
    dab = L.corr_bwd64(da.abs(), db.abs(), dgo.abs(), *CORR)
    dd = [R.delta_bf16x3(r, s, 441, C) for r, s in zip(dr, dab)]
    dense_of = lambda mutant: [T.inside(g, r, d) for g, r, d in zip(T.model_bwd(da, db, dgo, CORR, mutant=mutant), dr, dd)]
    assert all(ok for ok, _ in dense_of(None))
    dense = {m: dense_of(m) for m in T.X3_BWD_MUTANTS}
    sole = set()
    for name, a, b, go in T.x3_bwd_inputs(shape):
        refs = L.corr_bwd64(a, b, go, *CORR)
        sums = L.corr_bwd64(a.abs(), b.abs(), go.abs(), *CORR)
        ns = T.nnz_bwd(a, b, go, CORR)
        deltas = [T.delta_x3(r, s, n, C) for r, s, n in zip(refs, sums, ns)]
        for which, got, r, d, n, anyt in zip((1, 2), T.model_bwd(a, b, go, CORR), refs, deltas, ns, (any1, any2)):
            ok, ratio = T.inside(got, r, d)
            frac = T.small_count_fraction(n, anyt)
            print(f"  bf16x3 bwd {shape} {name} grad_input{which}: correct model, worst error / n_nz bound {ratio:.3g}; "
                  f"1 <= n_nz <= 4 on {frac:.3f} of the elements")
            assert ok and T.plus_zero_where(got, n) and frac >= 0.5
        s1, s2 = T.sole_terms_bwd(a, b, go, CORR)
        sole |= s1 | s2
        for mutant in T.X3_BWD_MUTANTS:
            for which, got, r, d, (dense_ok, dense_ratio) in zip((1, 2), T.model_bwd(a, b, go, CORR, mutant=mutant), refs, deltas, dense[mutant]):
                nz_ok, nz_ratio = T.inside(got, r, d)
                _verdict(f"bf16x3 bwd {shape} {name} grad_input{which} {mutant}", dense_ok, nz_ok, dense_ratio, nz_ratio)
                assert not nz_ok and dense_ok
    reach = T.reachable_planes(Hh, W)
    print(f"  {len(sole & reach)} of the {len(reach)} displacement planes with a term at {Hh} x {W} are some element's only term")
    assert sole >= reach


# ------------------------------------------------------------------ the pyramid
@pytest.mark.parametrize("shape", RP.SHAPES, ids=RP.shape_id)
def test_pyramid(shape):
    B, C, (Hh, W), (H2, W2), Lv = shape
    for name, f1, f2 in T.pyramid_inputs(shape):
        levels, S0 = RP.forward(f1, f2, Lv)
        n = T.nnz_pyramid(f1, f2)
        deltas = T.pyramid_bounds(levels, S0, C, n)
        counts = T.pooled_counts(n, Lv)
        got = T.model_pyramid(f1, f2, Lv)
        worst, per = RP.worst_ratio(got, levels, deltas)
        print(f"  pyramid {RP.shape_id(shape)} {name}: correct model, error / n_nz bound per level " + " ".join(f"{r:.3g}" for r in per))
        assert not RP.misses(got, levels, deltas)
        assert all(T.plus_zero_where(g, c) for g, c in zip(got, counts))
        if name != "channel_sparse":
            assert int(n.max()) == 1
            continue
        frac = T.small_count_fraction(n, torch.ones_like(n) > 0)
        sole = T.sole_terms_pyramid(f1, f2)
        print(f"  1 <= n_nz <= 4 on {frac:.3f} of level 0; {len(sole)} of {C} channels are some element's only term")
        assert frac >= 0.5 and sole == set(range(C))
        d1, d2 = RP.inputs(shape, seed=7 + C)                      # the dense inputs of tests/test_gpu_corr_pyramid.py
        dlev, dS0 = RP.forward(d1, d2, Lv)
        dden = RP.bounds(dlev, dS0, C)
        assert not RP.misses(T.model_pyramid(d1, d2, Lv), dlev, dden)
        for mutant in T.X3_MUTANTS:
            if mutant == "stale_l_slot" and C < 32:
                continue                                         # C = 8 has no fourth slot
            bad = T.model_pyramid(f1, f2, Lv, mutant)
            nz_ok, nz_ratio = not RP.misses(bad[:1], levels[:1], deltas[:1]), RP.worst_ratio(bad, levels, deltas)[0]
            dbad = T.model_pyramid(d1, d2, Lv, mutant)
            dense_ok, dense_ratio = not RP.misses(dbad, dlev, dden), RP.worst_ratio(dbad, dlev, dden)[0]
            _verdict(f"pyramid {RP.shape_id(shape)} {mutant}", dense_ok, nz_ok, dense_ratio, nz_ratio)
            pooled = ["REJECT" if RP.misses([g], [w], [d]) else "accept" for g, w, d in zip(bad[1:], levels[1:], deltas[1:])]
            print("    pooled levels (bit-equal to the pooling of level 0 in the GPU test): " + " ".join(pooled))
            assert not nz_ok                                     # at level 0
            if C >= 32:
                assert dense_ok


# ------------------------------------------------------------------ f16x2 forward
def test_f16x2_forward_narrow():
    """The model of tests/test_corr_contract_host.py at C = 320."""
    shape = T.F16_FWD_NARROW
    a, b = T.f16_fwd_inputs(shape)
    ref, delta, n = T.fwd_f16x2(a, b, wide=False)
    got = torch.from_numpy(H.model_fwd(a.numpy(), b.numpy()))
    ok, ratio = T.inside(got, ref, delta)
    print(f"  f16x2 fwd {shape}: correct model, worst error / n_nz bound {ratio:.3g}")
    assert ok and T.plus_zero_where(got, n)
    da, db = R.family_inputs(1, shape, seed=sum(shape))
    dref, ddelta, _ = T.fwd_f16x2(da, db, wide=False, n=shape[1])
    assert T.inside(torch.from_numpy(H.model_fwd(da.numpy(), db.numpy())), dref, ddelta)[0]
    nz_ok, nz_ratio = T.inside(torch.from_numpy(H.model_fwd(a.numpy(), b.numpy(), "drop_albh")), ref, delta)
    dense_ok, dense_ratio = T.inside(torch.from_numpy(H.model_fwd(da.numpy(), db.numpy(), "drop_albh")), dref, ddelta)
    _verdict(f"f16x2 fwd {shape} drop_albh", dense_ok, nz_ok, dense_ratio, nz_ratio)
    assert not nz_ok and dense_ok


@pytest.mark.parametrize("shape", [T.F16_FWD_NARROW, T.F16_FWD_WIDE], ids=sid)
def test_f16x2_forward_inputs_have_power(shape):
    a, b = T.f16_fwd_inputs(shape)
    n = T.nnz_fwd(a, b, CORR)
    frac = T.small_count_fraction(n, L.corr_fwd64(torch.ones(shape), torch.ones(shape), *CORR) > 0)
    print(f"  f16x2 fwd {shape}: 1 <= n_nz <= 4 on {frac:.3f} of the outputs with a term")
    assert frac >= 0.5


# ------------------------------------------------------------------ f16x2 backward
def test_f16x2_backward_shapes_are_the_contract_tests():
    assert T.F16_BWD_SHAPES == [G.BWD_NARROW[0], G.BWD_NARROW[1], G.BWD_WIDE[0], G.BWD_MULTI[2]]


_F16_SOLE = {}


@pytest.mark.parametrize("shape", T.F16_BWD_SHAPES, ids=sid)
def test_f16x2_backward(shape):
    B, C, Hh, W = shape
    a, b, go = T.f16_bwd_inputs(shape)
    one = torch.ones(shape)
    anys = [t > 0 for t in L.corr_bwd64(one, one, torch.ones(T._gshape(shape)), *CORR)]
    res = T.bwd_f16x2(a, b, go)
    for which, got, (r, d, n), anyt in zip((1, 2), T.model_bwd(a, b, go, CORR, "f16x2"), res, anys):
        ok, ratio = T.inside(got, r, d)
        frac = T.small_count_fraction(n, anyt)
        print(f"  f16x2 bwd {shape} grad_input{which}: correct model, worst error / n_nz bound {ratio:.3g}; "
              f"1 <= n_nz <= 4 on {frac:.3f} of the elements")
        assert ok and T.plus_zero_where(got, n) and frac >= 0.5
    _F16_SOLE[shape] = set.union(*T.sole_terms_bwd(a, b, go, CORR))
    # the mutant and the dense check on the first items (the items are independent; the rest cost the same passes again)
    a, b, go = a[:3], b[:3], go[:3]
    res = T.bwd_f16x2(a, b, go)
    da, db = R.family_inputs(1, a.shape, seed=sum(shape))
    dgo = R.grad_output("normal", go.shape, sum(shape))
    dres = T.bwd_f16x2(da, db, dgo, n=441)
    assert all(T.inside(g, r, d)[0] for g, (r, d, _) in zip(T.model_bwd(da, db, dgo, CORR, "f16x2"), dres))
    bad, dbad = T.model_bwd(a, b, go, CORR, "f16x2", "drop_glxh"), T.model_bwd(da, db, dgo, CORR, "f16x2", "drop_glxh")
    for which, g, (r, d, _), dg, (dr_, dd, _) in zip((1, 2), bad, res, dbad, dres):
        nz_ok, nz_ratio = T.inside(g, r, d)
        dense_ok, dense_ratio = T.inside(dg, dr_, dd)
        _verdict(f"f16x2 bwd {shape} grad_input{which} drop_glxh", dense_ok, nz_ok, dense_ratio, nz_ratio)
        assert not nz_ok
        # (the dense verdict is asserted where an element has all 441 terms: test_f16x2_backward_at_441_terms.  These images are
        # small, a middle pixel has terms_in_image(H, W) = 4 .. 84 of them, and with so few terms to cancel among the dense check
        # notices the mutant at some of them.)


def test_f16x2_backward_at_441_terms():
    """FlowNetC's 48 x 64 geometry, where the middle elements have all 441 terms: the dense check accepts the mutant, the n_nz bound
    on grad_sparse rejects it.  (Host only; the GPU cases keep the contract tests' shapes.)"""
    shape = (1, 64, 48, 64)
    assert T.terms_in_image(48, 64) == 441
    da, db = R.family_inputs(1, shape, seed=sum(shape))
    dgo = R.grad_output("normal", T._gshape(shape), sum(shape))
    dres = T.bwd_f16x2(da, db, dgo, n=441)
    a, b, go = T.f16_bwd_inputs(shape)
    res = T.bwd_f16x2(a, b, go)
    assert all(T.inside(g, r, d)[0] for g, (r, d, _) in zip(T.model_bwd(da, db, dgo, CORR, "f16x2"), dres))
    assert all(T.inside(g, r, d)[0] for g, (r, d, _) in zip(T.model_bwd(a, b, go, CORR, "f16x2"), res))
    bad, dbad = T.model_bwd(a, b, go, CORR, "f16x2", "drop_glxh"), T.model_bwd(da, db, dgo, CORR, "f16x2", "drop_glxh")
    for which, g, (r, d, _), dg, (dr_, dd, _) in zip((1, 2), bad, res, dbad, dres):
        nz_ok, nz_ratio = T.inside(g, r, d)
        dense_ok, dense_ratio = T.inside(dg, dr_, dd)
        _verdict(f"f16x2 bwd {shape} grad_input{which} drop_glxh", dense_ok, nz_ok, dense_ratio, nz_ratio)
        assert not nz_ok and dense_ok


def test_f16x2_backward_planes():
    """Every displacement plane with a term at any of the backward shapes is some element's only term at one of them."""
    for shape in T.F16_BWD_SHAPES:
        if shape not in _F16_SOLE:
            _F16_SOLE[shape] = set.union(*T.sole_terms_bwd(*T.f16_bwd_inputs(shape), CORR))
    reach = set.union(*(T.reachable_planes(*s[2:]) for s in T.F16_BWD_SHAPES))
    sole = set.union(*_F16_SOLE.values())
    print(f"  {len(sole & reach)} of the {len(reach)} displacement planes with a term at the f16x2 backward shapes are some element's only term")
    assert sole >= reach
