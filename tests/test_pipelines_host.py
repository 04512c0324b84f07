"""The two recipes of tests/pipelines_ref.py on the CPU, no GPU: what tests/test_gpu_pipelines.py relies on.

1. the inputs meet the conditions the comparisons need (sample coordinates away from integers, samples outside the image, a range
   map that is exact in float32, a mixed occlusion mask, a pyramid whose every level is at least 2 x 2);
2. the gather warp is the oracle's Resample2d, forward and backward, outside samples included;
3. the float32 compositions meet the acceptance rule against float64 (trivially: the rule is made of their error);
4. the rule has teeth: each wiring mutation of the float32 composition misses it in at least one compared tensor.

Both recipes run at the shapes of the GPU tests."""
import numpy as np
import pytest
import torch

import pipelines_ref as P

@pytest.fixture(scope="module")
def unsup():
    inp = P.unsup_inputs()
    return inp, P.run(P.unsup_loss, inp, torch.float64), P.run(P.unsup_loss, inp, torch.float32)


@pytest.fixture(scope="module")
def raft():
    inp = P.raft_inputs()
    return inp, P.run(P.mini_raft, inp, torch.float64), P.run(P.mini_raft, inp, torch.float32)


# ------------------------------------------------------------------ 1: the inputs
def test_unsupervised_inputs_meet_their_conditions(unsup):
    inp, o64, o32 = unsup
    P.check_unsup_inputs(inp)
    rm = {dt: P.torch_layers().range_map(torch.from_numpy(inp["flow21"]).to(dt)) for dt in (torch.float64, torch.float32)}
    for dt, r in rm.items():
        assert torch.equal(4 * r, (4 * r).round()), dt
    assert torch.equal(rm[torch.float64], rm[torch.float32].double())
    noc = o64["noc"]
    assert torch.equal(noc, o32["noc"].double()) and set(noc.unique().tolist()) == {0.0, 1.0}
    assert 0.2 <= float(noc.mean()) <= 0.9, float(noc.mean())


def test_mini_raft_inputs_meet_their_conditions(raft):
    inp, o64, _ = raft
    h, w = P.RAFT_SHAPE[1] // 8, P.RAFT_SHAPE[2] // 8
    assert P.RAFT_SHAPE[1] % 8 == 0 and P.RAFT_SHAPE[2] % 8 == 0
    for _ in range(P.RAFT_LEVELS - 1):
        h, w = h // 2, w // 2
    assert h >= 2 and w >= 2, (h, w)                  # corr_lookup_ref.compose divides by (size - 1)
    M = P.RL.header_macros()
    assert (P.RAFT_SHAPE[1] // 8) % M["FN2L_TILE_H"] and (P.RAFT_SHAPE[2] // 8) % M["FN2L_TILE_W"]     # ragged both ways
    # the refinement moves: the three flows differ, by a pixel of the coarse grid or more somewhere, and are not integers
    f = [o64["flow_up_%d" % i] for i in range(P.RAFT_ITERS)]
    for a, b in zip(f, f[1:]):
        assert float((a - b).abs().max()) > 8.0
    assert float((f[0] / 8 - (f[0] / 8).round()).abs().mean()) > 0.05
    for k, v in o64.items():
        assert torch.isfinite(v).all() and float(v.abs().max()) > 0, k


# ------------------------------------------------------------------ 2: the gather warp is Resample2d
def test_gather_warp_is_the_oracles_resample2d(oracle, unsup):
    """Forward, image gradient and flow gradient against the oracle on the recipe's own im2 and flow12.  The oracle is float32:
    both sides get the float32 coordinate fl32(x + flow) (the flow handed to the float64 gather is that coordinate minus x,
    exact), so what remains is the oracle's rounding after it --
      forward   4 products and 3 sums of terms that add up to at most max |img|: 8 * 2^-24 max |img|;
      grad_flow 4 C terms gamma * gO * I, three roundings each and 4 C sums: 32 * 2^-24 * sum |terms| <= 2 max |img| sum_c |gO_c|;
      grad_img  n contributions w * gO added in thread order, the weights of the truncated fraction (|w| <= 2 left of and
                above the image, where both corners are the border pixel): (n + 4) * 2^-24 * 3 sum |w gO|."""
    inp = unsup[0]
    img, flow = inp["im2"].astype(np.float32), inp["flow12"].astype(np.float32)
    N, C, H, W = img.shape
    outside = P.check_unsup_inputs(inp)
    go = np.random.default_rng(5).standard_normal(img.shape).astype(np.float32)
    xs, ys = np.arange(W, dtype=np.float32)[None, None, :], np.arange(H, dtype=np.float32)[None, :, None]
    exact_flow = np.stack([(xs + flow[:, 0]).astype(np.float64) - xs, (ys + flow[:, 1]).astype(np.float64) - ys], 1)
    ti = torch.from_numpy(img).double().requires_grad_(True)
    tf = torch.from_numpy(exact_flow).requires_grad_(True)
    out = P.gather_warp(ti, tf)
    gi, gf = torch.autograd.grad(out, (ti, tf), torch.from_numpy(go).double())
    mx = float(np.abs(img).max())
    err = np.abs(oracle.resample_fwd(img, flow).astype(np.float64) - out.detach().numpy())
    assert err.max() <= 8 * 2.0 ** -24 * mx, err.max()
    assert err[np.broadcast_to(outside[:, None], err.shape)].size >= 0.01 * err.size
    o_gi, o_gf = oracle.resample_bwd(img, flow, go)
    tol_f = 32 * 2.0 ** -24 * 2 * mx * np.abs(go).sum(1, keepdims=True)
    assert (np.abs(o_gf - gf.numpy()) <= tol_f).all(), float((np.abs(o_gf - gf.numpy()) / tol_f).max())
    assert np.abs(gf.numpy()[np.broadcast_to(outside[:, None], gf.shape)]).max() > 0      # the border's gradient is there
    S, = torch.autograd.grad(P.gather_warp(ti, tf), ti, torch.from_numpy(np.abs(go)).double())
    n, = torch.autograd.grad(P.gather_warp(ti, tf.detach().floor() + 0.5), ti, torch.ones_like(ti))   # 1/4 per corner
    tol_i = (4 * n.numpy() + 4) * 2.0 ** -24 * 3 * S.numpy()
    assert (np.abs(o_gi - gi.numpy()) <= tol_i).all(), float((np.abs(o_gi - gi.numpy()) / np.maximum(tol_i, 1e-300)).max())
    assert np.abs(gi.numpy()).max() > 1.0


# ------------------------------------------------------------------ 3: float32 meets the rule
@pytest.mark.parametrize("recipe", ["unsup", "raft"])
def test_float32_composition_meets_the_rule(recipe, request):
    _, o64, o32 = request.getfixturevalue(recipe)
    rep = P.rule_report(o32, o32, o64, recipe + " float32 ")
    for k, (err, bound, ratio) in rep.items():
        assert err <= bound and ratio in (0.0, 1.0), (k, err, bound)
        assert err <= 1e-3 * float(o64[k].abs().max()), k      # and float32 is a usable yardstick: nothing ill-conditioned


# ------------------------------------------------------------------ 4: the rule has teeth
@pytest.mark.parametrize("mutation", P.MUTATIONS_UNSUP + P.MUTATIONS_RAFT)
def test_the_rule_rejects_a_wiring_mutation(mutation, request):
    recipe, pipeline = ("unsup", P.unsup_loss) if mutation in P.MUTATIONS_UNSUP else ("raft", P.mini_raft)
    inp, o64, o32 = request.getfixturevalue(recipe)
    mutant = P.run(pipeline, inp, torch.float32, mutation=mutation)
    misses = P.rule_misses(mutant, o32, o64, mutation + " ")
    assert misses, f"{mutation} passes the rule in every tensor: the inputs are too tame"
