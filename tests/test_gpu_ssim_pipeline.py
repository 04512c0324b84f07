"""ARFlow's photometric recipe end to end: ``0.15 L1 + 0.85 SSIMLoss + CensusLoss`` on the warped second image
under the non-occluded mask, the HIP modules against the float64 composition by the rule of DESIGN.md 4.16, on the loss and the
three leaf gradients.  Inputs, warp and mask are those of tests/pipelines_ref.py's unsupervised recipe (N = 2, 3 x 36 x 132), imported
from there.  One mutation on the CPU -- the SSIM border swapped -- shows that the rule notices a wiring error.
"""
import numpy as np
import pytest
import torch

import pipelines_ref as P
import ssim_ref as R

W_L1, W_SSIM, W_TERNARY = 0.15, 0.85, 1.0
SSIM_MD = 1


def photometric(layers, ssim_loss, t):
    """{loss, l1, ssim, ternary, im1.grad, im2.grad, flow12.grad}; ``layers``: pipelines_ref.torch_layers() or hip_layers();
    ``ssim_loss(im1, im2_warped, mask)``: the composition or the module."""
    im1, im2, flow12 = (t[k].detach().clone().requires_grad_(True) for k in ("im1", "im2", "flow12"))
    im2_warped = layers.warp(im2, flow12.contiguous())
    noc = (layers.range_map(t["flow21"]) > 0.5).to(im1.dtype)
    l1 = ((im1 - im2_warped).abs() * noc).sum() / (im1.shape[1] * noc.sum() + 1e-6)
    ssim = ssim_loss(im1, im2_warped, noc)
    ternary = layers.census(im1, im2_warped, noc)
    loss = W_L1 * l1 + W_SSIM * ssim + W_TERNARY * ternary
    loss.backward()
    return {"loss": loss.detach(), "l1": l1.detach(), "ssim": ssim.detach(), "ternary": ternary.detach(), "im1.grad": im1.grad,
            "im2.grad": im2.grad, "flow12.grad": flow12.grad}


def _composition(dtype, border="zero"):
    inp = P.unsup_inputs()
    P.check_unsup_inputs(inp)
    return photometric(P.torch_layers(), lambda a, b, m: R.compose_loss(a, b, m, SSIM_MD, border), P._cast(inp, dtype, "cpu"))


@pytest.fixture(scope="module")
def references():
    return _composition(torch.float32), _composition(torch.float64)


def test_the_l1_term_has_no_sign_on_the_edge(references):
    """|im1 - warp| has a kink at 0: the inputs keep every masked difference far enough from it that float32 and float64 agree on
    the sign, so the rule compares one function."""
    inp = P._cast(P.unsup_inputs(), torch.float64, "cpu")
    diff = inp["im1"] - P.gather_warp(inp["im2"], inp["flow12"])
    assert float(diff.abs().min()) > 2.0 ** -20
    assert all(float(references[1][k]) > 0.01 for k in ("l1", "ssim", "ternary"))


def test_the_rule_notices_a_swapped_border(references):
    out32, out64 = references
    wrong = _composition(torch.float32, border="reflect")
    missed = P.rule_misses(wrong, out32, out64, "border swapped: ")
    assert "loss" in missed and "im1.grad" in missed, missed


@pytest.mark.gpu
def test_arflow_photometric_recipe_matches_float64(dev, references):
    from networks.ssim_package import SSIMLoss
    out32, out64 = references
    got = photometric(P.hip_layers(), SSIMLoss(md=SSIM_MD, border="zero"), P._cast(P.unsup_inputs(), torch.float32, dev))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert P.rule_misses(got, out32, out64, "ARFlow photometric: ") == []
