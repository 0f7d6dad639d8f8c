"""GPU: a plain bench.py run prints the headline line and measures nothing else; --full adds the per-kernel pricing.
Run at a small batch: this checks what the line holds, not how fast the step is."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "loss")
EXTRAS = ("roofline", "kernels", "attention_mfma_frac", "small_batch", "cpu_baseline")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "XVIT_BENCH_DRYRUN", "XVIT_FORCE_DIST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8", "--steps", "2", "--warmup", "1", *argv],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE), out.keys()
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    return out, r.stderr


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only():
    out, _ = _bench()
    assert not [k for k in EXTRAS if k in out]


@pytest.mark.gpu
def test_full_run_prices_the_kernels():
    out, err = _bench("--full", "--no-cpu-baseline", "--no-small-batch", "--detail")
    assert out["roofline"]["kernel"] in out["kernels"] and out["kernels"][out["roofline"]["kernel"]]["launches_per_step"] > 0
    assert "attn_fwd" in out["kernels"] and "attention_mfma_frac" in out
    assert "small_batch" not in out and "cpu_baseline" not in out
    assert re.search(r" x +\d+ +[\d.]+ us .* total +[\d.]+ ms/step", err), err[-2000:]     # a row of the --detail table
