"""bench.py without --full: set-up, warm-up, the timed steps and the line -- nothing that takes runs of its own.  CPU: the options
that only make sense beside the headline are refused without --full.  GPU: a plain run's line carries the headline keys and none of
--full's figures."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"kernels", "configs1_correlation_only", "roofline_mfma", "box", "ms_per_step_eager_with_events", "ms_per_step_autograd_modules",
             "cpu_baseline", "cpu_baseline_fast", "gpu_over_cpu", "flownet2c"}


@pytest.mark.parametrize("opt", ["--model", "--pmc"])
def test_extras_on_need_full(opt):
    """`--model on` / `--pmc on` ask for a figure beside the headline: without --full that is an argument error, before any GPU use."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", opt, "on"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "needs --full" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "8", "--warmup", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert HEADLINE <= set(line) and line["full"] is False
    assert line["unit"] == "image-pairs/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 8 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    assert not FULL_ONLY & set(line), FULL_ONLY & set(line)
    # the graded kernel's roofline from the event pairs inside the timed steps; the ceilings beside it are --full's
    roof = line["roofline"]
    assert roof["launch_ms"] > 0 and roof["achieved"] > 0 and roof["algorithmic_bytes"] == 93683712
    assert "copy_ceiling_GBps" not in roof and "traffic" not in roof
    (p,) = line["per_rank"]
    assert p["finite"] and p["ms_per_step"] > 0 and "corr_fwd_us_warm" not in p
