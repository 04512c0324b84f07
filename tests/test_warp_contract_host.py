"""The float64 references and bounds of tests/warp_contract_ref.py checked without a GPU: the oracle (the fp32 restatement of the
reference kernels, summing in a different order than the HIP kernels) must lie inside every bracket on every family x small shape
-- that validates the derivations --, the excluded share of grad_input1 cells stays under the cap in every case the GPU test uses,
mutants of the reference are caught by some family, and the kernels' host-side choices (tile height, sample pixels) are restated."""
import numpy as np
import pytest

import warp_contract_ref as R

WORST = {}
DIFF = [0, 0, 0]      # bilinear forward, the kernels' sequence against the oracle: elements that differ, elements, worst distance in ulp


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)


@pytest.mark.parametrize("case", R.CASES + R.FUSED_CASES, ids=lambda c: c.id)
def test_exclusion_cap(case):
    share = case.excluded_share()
    wild = float(R.positions(case.flow).wild.mean())
    print(f"{case.id}: wild pixels {100 * wild:.2f} %, excluded cells {100 * share:.2f} %")
    assert share <= R.EXCLUDED_CAP
    if case.family == "wild":
        assert 0 < wild <= 0.02
    if case.family in ("noise", "grid", "border", "window"):
        assert wild == 0 and share == 0


@pytest.mark.parametrize("case", R.SMALL_CASES, ids=lambda c: c.id)
def test_oracle_inside_the_brackets(oracle, case):
    for bilinear in (True, False):
        ref, delta, wild = case.fwd64(bilinear)
        got = oracle.resample_fwd(case.img, case.flow, case.ks, bilinear)
        # the oracle against the bound of ITS sequence (the BR term rounded twice); the kernels' sequence, below, against delta
        d_ref = R.resample_fwd64(case.img, case.flow, case.ks, bilinear, br_twice=True)[1]
        r = R.ratio_and_check(got, ref, d_ref, ~wild[:, None], f"{case.id} forward bilinear={bilinear}")
        _note("forward bilinear" if bilinear else "forward nearest", r)
        if bilinear:
            # the kernels' operation sequence restated in numpy has the oracle's bits wherever the BR terms vanish; elsewhere the
            # reference forms that term in fp32 (two roundings) and the kernels in double (one)
            seq, br_zero = case.seq32
            _note("forward bilinear, the kernels' sequence in numpy",
                  R.ratio_and_check(seq, ref, delta, ~wild[:, None], f"{case.id} the kernels' sequence in numpy"))
            eq = R.same_bits(seq, got)
            assert eq[br_zero].all()
            DIFF[0] += int((~eq).sum())
            DIFF[1] += eq.size
            DIFF[2] = max(DIFF[2], R.ulp_distance(seq, got))
    b = case.bwd64(False)
    gimg, gflow = oracle.resample_bwd(case.img, case.flow, case.gout, case.ks, True)
    r1 = R.ratio_and_check(gimg, b.gimg, b.gimg_delta, ~b.excluded[:, None], f"{case.id} grad_input1")
    r2 = R.ratio_and_check(gflow, b.gflow, b.gflow_delta, ~b.wild[:, None], f"{case.id} grad_flow")
    keep = ~b.reached & ~b.excluded[:, None]
    assert not gimg[keep].any(), "a cell no pixel reaches changed"
    _note("grad_input1", r1)
    _note("grad_flow", r2)
    print(f"{case.id}: oracle err / delta: grad_input1 {r1:.3f}, grad_flow {r2:.3f}")
    assert max(r1, r2) <= 1.0


@pytest.mark.parametrize("shape", R.CHNORM_SHAPES)
def test_oracle_channelnorm_inside_the_brackets(oracle, shape):
    x = R.chnorm_input(shape)
    out = oracle.chnorm_fwd(x)
    ref, delta = R.chnorm_fwd64(x)
    r1 = R.ratio_and_check(out, ref, delta, None, f"{shape} chnorm forward")
    assert out[0, 0, 0, 0] == 0
    go = np.ascontiguousarray(R.graded((shape[0], 2) + shape[2:], 0)[:, 1:])
    gin = oracle.chnorm_bwd(x, out, go)
    ref, delta = R.chnorm_bwd64(x, out, go)
    r2 = R.ratio_and_check(gin, ref, delta, None, f"{shape} chnorm backward")
    assert not np.isnan(gin).any() and not gin[0, :, 0, 0].any()
    _note("chnorm forward", r1)
    _note("chnorm backward", r2)
    print(f"{shape}: oracle err / delta: chnorm forward {r1:.3f}, backward {r2:.3f}")


def test_report_oracle_ratios():
    """the worst oracle err / delta per quantity over the tests above (all <= 1 by their assertions)"""
    for k in sorted(WORST):
        print(f"oracle worst err / delta, {k}: {WORST[k]:.3f}")
    print(f"bilinear forward, the kernels' operation sequence against the oracle: {DIFF[0]} of {DIFF[1]} elements differ, at most {DIFF[2]} ulp")
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------ teeth: mutants of the reference
def _caught(fn, cases):
    """ids of the cases in which the oracle's output leaves the MUTANT reference's bracket"""
    hit = []
    for case in cases:
        try:
            fn(case)
        except AssertionError:
            hit.append(case.id)
    return hit


def test_mutants_are_caught(oracle):
    small = [c for c in R.SMALL_CASES if c.family != "follow" and c.img_shape[2] * c.img_shape[3] <= 35 * 132]

    def fwd(mut, bilinear):
        def f(case):
            ref, delta, wild = R.resample_fwd64(case.img, case.flow, case.ks, bilinear, mut=(mut,))
            R.ratio_and_check(oracle.resample_fwd(case.img, case.flow, case.ks, bilinear), ref, delta, ~wild[:, None], mut)
        return f

    def bwd(mut, what):
        def f(case):
            b = R.resample_bwd64(case.img, case.flow, case.gout, case.ks, mut=(mut,))
            gimg, gflow = oracle.resample_bwd(case.img, case.flow, case.gout, case.ks, True)
            if what == "gimg":
                R.ratio_and_check(gimg, b.gimg, b.gimg_delta, ~b.excluded[:, None], mut)
            else:
                R.ratio_and_check(gflow, b.gflow, b.gflow_delta, ~b.wild[:, None], mut)
        return f

    rect = [c for c in small if c.img_shape[2:] != (c.H, c.W)]
    batched = [c for c in small if c.img_shape[0] > 1]
    found = {
        "floored scatter alpha": _caught(bwd("floor_scatter", "gimg"), small),
        "gather clamped with the image dims (forward)": _caught(fwd("image_clamp", True), rect),
        "gather clamped with the image dims (grad_flow)": _caught(bwd("image_clamp", "gflow"), rect),
        "nearest by rint": _caught(fwd("rint", False), small),
        "corners of the neighbouring batch item (forward)": _caught(fwd("batch", True), batched),
        "corners of the neighbouring batch item (grad_flow)": _caught(bwd("batch", "gflow"), batched),
        "a dropped corner term of grad_flow": _caught(bwd("drop", "gflow"), small),
    }
    for name, hit in found.items():
        print(f"mutant '{name}': caught in {len(hit)} cases, e.g. {hit[:3]}")
    assert all(found.values()), [k for k, v in found.items() if not v]
    # Floored and truncated fractions differ only at xf < 0, where the clamp sends both corners to cell 0: in exact arithmetic the cell
    # gets the same sum (the weights add up to the same), so only the roundings and the sum of |terms| differ -- it is the `wild`
    # family that shows them: xf = 2^31 - 128 is not wild, int(xf) saturates, the truncated fraction is -128 and the floored one 0.
    assert any("wild" in i for i in found["floored scatter alpha"])
    assert any("grid" in i for i in found["nearest by rint"])


# ------------------------------------------------------------------ the families produce what they are for
def test_special_positions_are_produced():
    c = R.Case((1, 4, 35, 132), None, 1, "grid")
    P = R.positions(c.flow)
    assert (P.fa == 0.5).any() and (P.fa == 0).any() and (P.fa == np.float32(1)).any()          # fa == 1: xf just below 0
    assert ((P.xf > -1) & (P.xf < 0)).any() and ((P.ta < 0) & (P.fa > 0)).any()
    assert (np.signbit(c.flow) & (c.flow == 0)).any()                                          # -0.0
    assert ((c.flow[:, 0] == np.float32(-2.0 ** -25)) & (P.fa == 0) & (P.xf >= 1)).any()        # x + dx rounds to x
    assert ((P.fa < 0.5) & (P.fa > 0.4999)).any() and ((P.fa > 0.5) & (P.fa < 0.5001)).any() and ((P.fa < 1) & (P.fa > 0.9999)).any()
    c = R.Case((2, 2, 6, 9), (9, 13), 1, "border")
    P = R.positions(c.flow)
    for v in (-1.0, -0.5, 0.0, 12.0, 12.5, 13.0, 8.0, 8.5, 9.0):
        assert (P.xf == np.float32(v)).any(), v
    for v in (-1.0, 0.0, 8.0, 9.0, 5.0, 6.0):
        assert (P.yf == np.float32(v)).any(), v
    c = R.Case((1, 4, 35, 132), None, 1, "window")
    P = R.positions(c.flow)
    xs = np.arange(132)[None, None, :]
    X0 = xs // 64 * 64
    for v in (X0 - 17, X0 - 16, X0 + 79, X0 + 80):
        assert (P.xf == v.astype(np.float32)).any()
    assert ((P.xf > X0 - 16) & (P.xf < X0 - 15.999)).any() and ((P.xf < X0 + 79) & (P.xf > X0 + 78.999)).any()


def test_tile_height_and_sample_pixels_restated():
    """tile_height() and tile_flow_sample() of csrc/resample2d.hip, restated here on their own and compared with what the families use"""
    B, C, H, W = R.BIG_SHAPE
    tiles_x = (W + 63) // 64
    assert B * tiles_x * ((H + 31) // 32) == 513 and B * tiles_x * ((H + 47) // 48) == 342      # two rounds of 32-row tiles, one of 48
    assert R.tile_height(B, H, tiles_x) == 48
    assert R.tile_height(8, 384, 8) == 48 and R.tile_height(2, 33, 2) == 32 and R.tile_height(1, 16, 1) == 32
    for shape in R.TILED_SHAPES + R.FOLLOW_WIDE + R.FUSED_SHAPES[:2]:
        assert R.tileable(shape[2], shape[3], shape[2], shape[3])
    assert not R.tileable(17, 33, 17, 33) and not R.tileable(8, 36, 8, 36) and not R.tileable(15, 32, 15, 32)
    for H, W, TH in ((35, 132, 32), (16, 32, 32), (96, 10944, 48)):
        S = R.sample_pixels(H, W, TH)
        assert len(S) == ((H + TH - 1) // TH) * ((W + 63) // 64)
        for (ty, tx), pts in S.items():
            for q, (x, y) in enumerate(pts):
                assert x == min(tx * 64 + 16 + (q & 1) * 32, W - 1) and y == min(ty * TH + TH // 4 + (q >> 1) * (TH // 2), H - 1)
    # the families put their values on these pixels
    w = R.Case((1, 3, 35, 132), None, 1, "window").flow
    for pts in R.sample_pixels(35, 132).values():
        assert all(not w[0, :, y, x].any() for x, y in pts)


@pytest.mark.parametrize("c3", [True, False], ids=["C=3", "C!=3"])
def test_follow_family_covers_the_table(c3):
    """Over the `follow` cases the GPU test runs, separately for C = 3 (resample_bwd_c3x) and C != 3 (resample_bwd_tiled): every
    translation x direction (x, y, both) x sample-pixel setting (all agree, one outlier, two outliers, middle pair 7.9 px apart, 8.1 px
    apart) lands on a tile whose four sample pixels are distinct pixels, and the flow at those pixels is what the setting says."""
    seen = set()
    for case in R.CASES:
        B, C, H, W = case.img_shape
        if case.family != "follow" or (C == 3) != c3:
            continue
        tiles_y, tiles_x = (H + 31) // 32, (W + 63) // 64
        for b in range(B):
            for (ty, tx), pts in R.sample_pixels(H, W).items():
                if len(set(pts)) < 4:
                    continue        # a ragged tile whose sample pixels coincide: later values overwrite earlier ones
                T, direc, setting, rot = R.follow_plan(b, ty, tx, tiles_y, tiles_x, case.seed)
                for comp in (0, 1):
                    tc = np.float32(T) if direc in (2, comp) else np.float32(0)
                    vals = [case.flow[b, comp, y, x] for x, y in pts]
                    if setting == 0:
                        assert all(v == tc for v in vals)
                    elif setting in (1, 2):
                        assert sum(1 for v in vals if v == tc) == 4 - setting and sum(1 for v in vals if not abs(v) < 1e29) == setting
                    elif setting in (3, 4):
                        mid = sorted(vals)[1:3]
                        assert mid[0] == tc and (mid[1] - mid[0] < 8) == (setting == 3)
                seen.add((T, direc, setting))
    want = {(T, d, s) for T in R.TRANSLATIONS for d in range(3) for s in range(5)}
    assert want <= seen, sorted(want - seen)[:10]
    print(f"follow, {'C = 3' if c3 else 'C != 3'}: {len(seen)} of {R.FOLLOW_TABLE} table entries on whole tiles")
