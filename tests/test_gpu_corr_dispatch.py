"""FN2_CORR_AUTO runs the first kernel of the plan fn2_debug_correlation_plan reports (tests/test_corr_dispatch_host.py pins the
plans): for one call per row of the dispatcher's table that a selector can name, forward and backward, AUTO's result has the bits of
that kernel called by name -- and, on FlowNetC's shape, not the bits of the plan's second kernel, so the comparison can tell two
candidates apart.  The smallest shapes of each kernel's domain; the dense forward needs the 192 tiles AUTO asks for."""
import pytest
import torch

import fn2_capi
from corr_dispatch_cases import DENSE4, FLOWNETC, K3, P20, WIDE, md

pytestmark = pytest.mark.gpu

SELECTOR = {"H16": fn2_capi.FN2_CORR_MFMA_F16X2, "F16X2": fn2_capi.FN2_CORR_MFMA_F16X2, "MFMA_F32": fn2_capi.FN2_CORR_MFMA_F32,
            "DENSE": fn2_capi.FN2_DEBUG_CORR_DENSE, "DIRECT": fn2_capi.FN2_CORR_DIRECT}
# (dtype, forward shape, backward shape, parameters, the first kernel of both plans)
CASES = [
    (torch.float32, FLOWNETC, FLOWNETC, P20, "F16X2"),
    (torch.float32, WIDE, WIDE, P20, "F16X2"),
    (torch.float32, (1, 32, 2, 2), (1, 32, 2, 2), md(4), "MFMA_F32"),
    (torch.float16, (1, 128, 2, 8), FLOWNETC, P20, "H16"),
    (torch.bfloat16, (1, 128, 2, 8), FLOWNETC, P20, "H16"),
    (torch.float32, (8, 4, 48, 64), (8, 4, 48, 64), DENSE4, "DENSE"),
    (torch.float32, (1, 3, 5, 6), (1, 3, 5, 6), K3, "DIRECT"),
]


def _inputs(dev, dtype, shape, params, backward):
    g = torch.Generator(device="cpu").manual_seed(sum(shape) + 31 * backward)
    a, b = (torch.randn(shape, generator=g).to(dev, dtype) for _ in range(2))
    if not backward:
        return a, b
    go = torch.randn((shape[0],) + fn2_capi.correlation_output_shape(shape[2], shape[3], *params), generator=g).to(dev, dtype)
    return a, b, go


def _run(tensors, params, algo):
    if len(tensors) == 2:
        return (fn2_capi.correlation_forward(*tensors, *params, algo=algo),)
    return fn2_capi.correlation_backward(*tensors, *params, algo=algo)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % (str(c[0]).split(".")[1], c[4]))
def test_auto_runs_the_first_kernel_of_the_plan(dev, case, backward):
    dtype, fwd_shape, bwd_shape, params, first = case
    shape = bwd_shape if backward else fwd_shape
    tensors = _inputs(dev, dtype, shape, params, backward)
    ptrs = [t.data_ptr() for t in tensors] + [tensors[0].data_ptr()] * 2   # (the gradients are torch allocations like the inputs)
    plan = fn2_capi.correlation_plan("backward" if backward else "forward", fn2_capi._dtype_code(tensors[0]), shape, *params, ptrs=ptrs)
    assert plan[0] == first, plan
    auto = _run(tensors, params, fn2_capi.FN2_CORR_AUTO)
    named = _run(tensors, params, SELECTOR[first])
    for x, y in zip(auto, named):
        assert torch.isfinite(x.float()).all() and torch.equal(x, y), (first, (x.float() - y.float()).abs().max().item())
    if shape == FLOWNETC and dtype == torch.float32:
        assert plan[1] == "MFMA_F32"
        other = _run(tensors, params, SELECTOR[plan[1]])
        assert not any(torch.equal(x, y) for x, y in zip(auto, other)), "the f16 split and the fp32 chain round differently"
