"""pipeline.reserve_hw_queues: four or more lanes get eight hardware queues whether GPU_MAX_HW_QUEUES is absent or spells out the runtime's default; a larger value
stays, HFASR_HW_QUEUES pins one.  Every case runs in a fresh child process that never initialises the GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import os, sys
sys.path.insert(0, {root!r})
from huggingface_asr_amd.pipeline import reserve_hw_queues
print(reserve_hw_queues(int(sys.argv[1])), os.environ.get("GPU_MAX_HW_QUEUES"))
"""


def _run(lanes, exported=None, pin=None):
    env = dict(os.environ)
    env.pop("GPU_MAX_HW_QUEUES", None)
    env.pop("HFASR_HW_QUEUES", None)
    if exported is not None:
        env["GPU_MAX_HW_QUEUES"] = exported
    if pin is not None:
        env["HFASR_HW_QUEUES"] = pin
    p = subprocess.run([sys.executable, "-c", SCRIPT.format(root=ROOT), str(lanes)], env=env, capture_output=True, text=True)
    if p.returncode:
        return p.stderr.strip().splitlines()[-1]
    out = p.stdout.split()
    return int(out[0]), out[1]


@pytest.mark.parametrize("lanes,exported,pin,want", [
    (4, None, None, (8, "8")),            # absent -> 8
    (4, "4", None, (8, "8")),             # the runtime's default, exported: raised
    (6, "4", None, (8, "8")),             # never above 8 on its own
    (4, "16", None, (16, "16")),          # never lowered
    (4, "8", None, (8, "8")),
    (4, None, "4", (4, "4")),             # the pin wins over the lanes' need ...
    (4, "8", "4", (4, "4")),              # ... and over an exported value
    (2, None, "12", (12, "12")),
    (3, None, None, (4, "None")),         # three lanes fit the default: unchanged
    (3, "4", None, (4, "4")),
    (3, "16", None, (16, "16")),
])
def test_queue_count_for_lanes(lanes, exported, pin, want):
    assert _run(lanes, exported, pin) == want


def test_a_pin_outside_the_allowed_range_is_refused():
    assert "HFASR_HW_QUEUES" in _run(4, None, "64")
    assert "HFASR_HW_QUEUES" in _run(4, None, "0")
