"""bench.py's forward headline as its own process: a plain run does only what the headline needs (set up, warm up, time the steps, print one line), and --full adds
the legs after the timed region."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_headline_only():
    rec = _bench()
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["unit"] == "audio-seconds/sec" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["steps_in_flight"] == 4
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["secondary"] is None and rec["train_dp"] is None
    assert rec["config"]["one_step_at_a_time"] is None and rec["one_step_ms"] is None and rec["one_step_value"] is None


def test_full_run_adds_the_one_step_comparison():
    rec = _bench("--full", "--no-kernel-events", "--no-cpu-baseline", "--no-secondary")
    assert rec["value"] > 0 and rec["steps_in_flight"] == 4
    single = rec["config"]["one_step_at_a_time"]
    assert single is not None and single["ms_per_step"] > 0 and single["value"] > 0
    assert rec["one_step_ms"] == single["ms_per_step"] and rec["one_step_value"] == single["value"]
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["secondary"] is None
