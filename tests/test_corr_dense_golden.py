"""The dense stride-1 configuration Correlation(md, 1, md, 1, 1) against what the REFERENCE's own device code produced
(tests/golden/corrdense_*.npz, written by tests/golden/make_golden_corr_dense.py): on the CPU the restated oracle equals the
fixture bit for bit (its standing claim, extended to this configuration); on the GPU the HIP kernels -- FN2_CORR_AUTO, which
runs csrc/correlation_dense.hip here, and FN2_CORR_DIRECT -- agree with it within the tolerance
tests/test_gpu_parity.py::test_correlation_golden applies to the same kind of fixture."""
import os

import numpy as np
import pytest

from conftest import golden_files, max_abs

FILES = golden_files("corrdense")


def test_corrdense_fixtures_present():
    assert len(FILES) == 3, FILES
    for path in FILES:
        assert os.path.getsize(path) < 1000000, path
        g = np.load(path)
        md = int(g["params"][0])
        assert tuple(int(v) for v in g["params"]) == (md, 1, md, 1, 1) and 1 <= md <= 4
        B, C, H, W = g["in1"].shape
        assert g["out"].shape == (B, (2 * md + 1) ** 2, H, W) == g["gout"].shape
        assert g["g1"].shape == g["in1"].shape == g["g2"].shape and g["out"].dtype == np.float32


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_oracle_equals_reference_on_dense_parameters(oracle, path):
    g = np.load(path)
    params = tuple(int(v) for v in g["params"])
    out = oracle.corr_fwd(g["in1"], g["in2"], *params)
    assert np.array_equal(out.view(np.int32), g["out"].view(np.int32))
    g1, g2 = oracle.corr_bwd(g["in1"], g["in2"], g["gout"], *params)
    assert np.array_equal(g1.view(np.int32), g["g1"].view(np.int32))
    assert np.array_equal(g2.view(np.int32), g["g2"].view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
def test_hip_matches_reference_on_dense_parameters(dev, path):
    import torch

    import fn2_capi
    from test_gpu_parity import TOL
    g = np.load(path)
    params = tuple(int(v) for v in g["params"])
    a, b, go = (torch.from_numpy(g[k]).to(dev) for k in ("in1", "in2", "gout"))
    for algo in (fn2_capi.FN2_CORR_AUTO, fn2_capi.FN2_DEBUG_CORR_DENSE, fn2_capi.FN2_CORR_DIRECT):
        out = fn2_capi.correlation_forward(a, b, *params, algo=algo, out=torch.full(g["out"].shape, float("nan"), device=dev))
        g1, g2 = fn2_capi.correlation_backward(a, b, go, *params, algo=algo,
                                               out=(torch.full_like(a, float("nan")), torch.full_like(b, float("nan"))))
        e = [max_abs(t.cpu().numpy(), g[k]) for t, k in ((out, "out"), (g1, "g1"), (g2, "g2"))]
        print(f"  {os.path.basename(path)} algo {algo}: max abs error out {e[0]:.3g}, g1 {e[1]:.3g}, g2 {e[2]:.3g}")
        assert max(e) <= TOL, (algo, e)
