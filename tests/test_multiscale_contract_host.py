"""CPU side of the MultiScale loss contract (tests/multiscale_ref.py): the float32 emulation of csrc/multiscale_loss.hip in its summation
order stays inside every bound at every geometry the GPU test runs, none of the seeded inputs leaves an element undetermined, and each of
a list of deliberately wrong kernels is caught by a named check at a named shape of the GPU test -- so a shape or a check that goes
missing there shows here."""
import numpy as np
import pytest

import multiscale_ref as R

# (B, H, W, start_scale, num_scales): the geometries of tests/test_gpu_multiscale_contract.py
SHAPES = [(2, 100, 202, 4, 5), (2, 100, 200, 4, 5), (1, 37, 70, 1, 5), (2, 48, 80, 2, 4), (1, 64, 96, 8, 3), (1, 70, 300, 16, 5),
          (3, 16, 16, 4, 1), (1, 130, 70, 4, 5), (2, 96, 96, 1, 3), (0, 32, 32, 4, 2)]
EXACT_SHAPES = [(2, 100, 202, 4, 5), (1, 37, 70, 1, 5)]
DIV_FLOW = 0.05

_cache = {}


def sid(shape):
    return "%dx%dx%d_s%d_n%d" % tuple(shape)


def seeded(shape):
    if shape not in _cache:
        target, outs, w = R.seeded_inputs(shape)
        _cache[shape] = (target, outs, w, R.Ref(target, outs, w, shape[3], DIV_FLOW))
    return _cache[shape]


def exact(shape):
    if ("exact", shape) not in _cache:
        target, outs, w, df = R.exact_inputs(shape)
        _cache[("exact", shape)] = (target, outs, w, df, R.Ref(target, outs, w, shape[3], df))
    return _cache[("exact", shape)]


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_seeded_inputs_leave_nothing_undetermined(shape):
    """A condition on the inputs, not a measurement: with e_m / |d| around 1e-7 no element may sit inside its own bound.  (A seed that
    produces one is replaced, the cap stays 0.)"""
    ref = seeded(shape)[3]
    assert ref.undetermined_count() == 0
    if shape == (1, 70, 300, 16, 5):
        assert [d.size for d in ref.d[3:]] == [0, 0]                    # k = 128, 256 > H: levels without elements
    if shape == (2, 96, 96, 1, 3):
        assert ref.nblocks == 1152                                      # five trips of the last workgroup's strided loop


@pytest.mark.parametrize("fma", [False, True], ids=["mul_add", "fma"])
@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_emulation_is_inside_every_bound(shape, norm, fma):
    target, outs, w, ref = seeded(shape)
    sums, loss_epe, grads = R.emulate(target, outs, w, shape[3], DIV_FLOW, norm, fma=fma)
    for name, rep in R.run_checks(ref, norm, sums, loss_epe, grads).items():
        assert rep.ok, rep
    if shape[0] == 0 or shape == (1, 70, 300, 16, 5):
        empty = [i for i in range(ref.ns) if ref.d[i].size == 0]
        assert empty and all(sums[i] == 0 and sums[ref.ns + i] == 0 for i in empty)


@pytest.mark.parametrize("fma", [False, True], ids=["mul_add", "fma"])
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=sid)
def test_exact_case(shape, fma):
    """On the dyadic inputs the order of the additions cannot matter: L1 sums and norm-1 gradients bit for bit, planted zeros give 0."""
    target, outs, w, df, ref = exact(shape)
    planted = sum(int((d == 0).sum()) for d in ref.d)
    assert planted >= 20, planted
    for i in range(ref.ns):                                             # nothing but the planted zeros is undetermined
        assert np.array_equal(ref.undetermined(i, 1), ref.d[i] == 0)
        assert np.array_equal(ref.undetermined(i, 2), (ref.d[i] == 0).all(axis=1))
    s1, le1, g1 = R.emulate(target, outs, w, shape[3], df, 1, fma=fma)
    s2, le2, g2 = R.emulate(target, outs, w, shape[3], df, 2, fma=fma)
    rep = R.check_exact(ref, s1, g1, g2)
    assert rep.ok, rep
    for norm, (s, le, g) in ((1, (s1, le1, g1)), (2, (s2, le2, g2))):
        for rep in R.run_checks(ref, norm, s, le, g).values():
            assert rep.ok, rep


# mutant -> (inputs, shape, norm, check) that catches it, found by running every mutant through every check at every shape above.
# A mutant that nothing catches means a missing shape: add the shape, not a tolerance.
CAUGHT_BY = {
    "drop_last":      ("seeded", (1, 37, 70, 1, 5), 1, "grads"),        # start_scale 1: the cell's only element
    "partial_edge":   ("seeded", (2, 100, 202, 4, 5), 1, "sums"),       # ragged in both directions
    "three_children": ("seeded", (2, 48, 80, 2, 4), 1, "grads"),
    "wrong_plane":    ("seeded", (1, 130, 70, 4, 5), 1, "grads"),
    "gw_next_n":      ("seeded", (1, 64, 96, 8, 3), 1, "grads"),
    "l2_d0_both":     ("seeded", (3, 16, 16, 4, 1), 2, "grads"),
    "sign0_plus":     ("exact", (2, 100, 202, 4, 5), 1, "exact"),       # only a planted d == 0 can tell
    "first_256":      ("seeded", (2, 96, 96, 1, 3), 1, "sums"),         # the only shape with more than 256 workgroups
    "no_div_flow":    ("seeded", (2, 100, 200, 4, 5), 2, "loss_epe"),
}


def test_every_mutant_has_an_entry():
    assert set(CAUGHT_BY) == set(R.ALL_MUTANTS)


@pytest.mark.parametrize("mutant", R.ALL_MUTANTS)
def test_mutant_is_caught(mutant):
    kind, shape, norm, check = CAUGHT_BY[mutant]
    assert shape in (EXACT_SHAPES if kind == "exact" else SHAPES)
    if kind == "exact":
        target, outs, w, df, ref = exact(shape)
        _, _, g1 = R.emulate(target, outs, w, shape[3], df, 1, mutant=mutant)
        s1, _, _ = R.emulate(target, outs, w, shape[3], df, 1, mutant=mutant)
        _, _, g2 = R.emulate(target, outs, w, shape[3], df, 2, mutant=mutant)
        rep = R.check_exact(ref, s1, g1, g2)
    else:
        target, outs, w, ref = seeded(shape)
        sums, loss_epe, grads = R.emulate(target, outs, w, shape[3], DIV_FLOW, norm, mutant=mutant)
        rep = R.run_checks(ref, norm, sums, loss_epe, grads)[check]
    assert not rep.ok, (mutant, rep)
    assert "level" in rep.worst and "got" in rep.worst and "want" in rep.worst and "bound" in rep.worst, rep.worst


def test_first_256_mutant_is_invisible_below_257_workgroups():
    """Why the 1152-workgroup shape is in the list: at every other shape the mutant computes the same bits."""
    for shape in SHAPES[:-1]:
        if shape == (2, 96, 96, 1, 3):
            continue
        target, outs, w, _ = seeded(shape)
        a = R.emulate(target, outs, w, shape[3], DIV_FLOW, 1)
        b = R.emulate(target, outs, w, shape[3], DIV_FLOW, 1, mutant="first_256")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("shape", SHAPES[:-1], ids=sid)
def test_sum_bounds_notice_one_dropped_element(shape):
    """The bounds of the sums are worst-case sums of per-element bounds, far above the error a correct kernel makes; what they are for is
    the reduction: at every shape and level they stay below the level's mean term, so one typical element lost or counted twice on the
    way through lanes, waves and workgroups shows."""
    ref = seeded(shape)[3]
    S, Bd = ref.sums_and_bounds()
    for i in range(ref.ns):
        if ref.d[i].size:
            assert Bd[i] < S[i] / ref.d[i].size and Bd[ref.ns + i] < S[ref.ns + i] / (ref.d[i].size // 2), (i, Bd, S)


def test_unit_weight_is_the_host_codes_expression():
    """gw / coef: a float64 product and quotient rounded once -- not a float32 quotient."""
    w, n = 0.32 / 4, 2 * 2 * 25 * 50
    assert R.unit_weight(w, 1.0, n) == np.float32(np.float64(np.float32(w)) / n)
    assert R.unit_weight(w, 3.0, 0) == 0
    assert R.gamma(3) == 3 * R.U / (1 - 3 * R.U)
