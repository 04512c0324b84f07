"""bench.py --dump-outputs: the outputs of the last timed step, as .npy files, bounded in size and the same from run to run, so that
two builds of the project can be compared output for output.  CPU: the sampling and the files (the step's buffers filled on the host).
GPU: the option end to end, against the same step run again in this process on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = {"correlation_output", "correlation_grad_input1", "correlation_grad_input2", "resample2d_output", "channelnorm_output",
         "channelnorm_grad_input", "resample2d_grad_input1", "resample2d_grad_input2"}


def _expected(t, entry):
    """What --dump-outputs writes for tensor `t` given its JSON entry: the whole tensor, or the seeded sample of its flat elements."""
    flat = t.detach().cpu().reshape(-1).numpy()
    if "sample" not in entry:
        return t.detach().cpu().numpy()
    s = entry["sample"]
    pos = np.sort(np.random.default_rng(s["seed"]).choice(flat.size, s["elements"], replace=False))
    return flat[pos]


def test_dump_outputs_files_are_bounded_and_reproducible(tmp_path):
    hp = bench.HotPath(torch.device("cpu"), seed=1234)
    c = bench.CORR
    g = torch.Generator().manual_seed(5)
    hp.out = torch.randn(c["B"], 441, c["H"], c["W"], generator=g)
    hp.g1, hp.g2 = torch.randn(hp.in1.shape, generator=g), torch.randn(hp.in2.shape, generator=g)
    for t in (hp.warped, hp.norm, hp.gdiff, hp.gimg, hp.gflow):
        t.copy_(torch.randn(t.shape, generator=g))
    a = hp.dump_outputs(str(tmp_path / "a"))
    b = hp.dump_outputs(str(tmp_path / "b"))
    assert set(a["arrays"]) == NAMES and a["arrays"] == b["arrays"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in NAMES)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6
    outs = hp.outputs()
    for name, entry in a["arrays"].items():
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, y)
        assert entry["shape"] == list(outs[name].shape)
        assert np.array_equal(x, _expected(outs[name], entry))
        assert ("sample" in entry) == (outs[name].numel() > bench.DUMP_MAX_ELEMS)
    assert "sample" in a["arrays"]["correlation_output"]


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_timed_steps(tmp_path, dev):
    """One process: `--steps 3` timed steps, the dump of the last one; the same step run here on HotPath's seeded inputs gives the
    same arrays (to the last bits that atomically accumulated gradients may differ in)."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                        "--model", "off", "--pmc", "off", "--placement", "off", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    arrays = line["dump_outputs"]["arrays"]
    assert set(arrays) == NAMES
    assert sum(os.path.getsize(out / (n + ".npy")) for n in NAMES) <= 64 * 10 ** 6
    hp = bench.HotPath(dev, seed=1234)
    hp.step()
    torch.cuda.synchronize()
    for name, t in hp.outputs().items():
        got, want = np.load(out / (name + ".npy")), _expected(t, arrays[name])
        assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), name
        assert float(np.abs(got.astype(np.float64) - want).max()) <= 1e-5 * max(1.0, float(np.abs(want).max())), name
