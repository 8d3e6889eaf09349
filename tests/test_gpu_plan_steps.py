"""The launch lists of the fused YOLOv8 / YOLOv5 / YOLO11 plans are what ``tests/golden/plan_steps.json`` records: for every case of
``tools/plan_steps.py`` (the smallest plans that reach every branch of the graph builders in csrc/rva_plan.hip) the anchors, the rows
of the head tensor, the number of steps and of tunable steps, ``quiet_step``, whether the detect branches have lanes, and for every
step its description (kernel, shape, row window) and its row window.  The plans are only created, nothing runs.  The record is the
library's own output from before the builders were rebuilt from shared parts; a change that moves, drops, adds or reshapes a launch
has to regenerate it (``python tools/plan_steps.py``) and show the difference."""
import functools
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("plan_steps", ROOT / "tools" / "plan_steps.py")
plan_steps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_steps)


@functools.lru_cache(maxsize=None)
def _golden():
    """The record, read when the first test needs it and shared; never modified.  Not at import: parsed at collection, its few
    thousand lists would live through the whole session and move the moments at which the interpreter collects garbage in the
    tests that run before this file -- and ``test_gpu_api.py`` has a hipGraph capture that does not survive every such moment."""
    return json.loads(plan_steps.GOLDEN.read_text())["cases"]


def test_golden_covers_the_cases():
    assert list(_golden()) == list(plan_steps.CASES)


@pytest.mark.parametrize("name", list(plan_steps.CASES))
def test_step_list(name):
    got = json.loads(json.dumps(plan_steps.describe(plan_steps.build_plan(name))))      # tuples -> lists, as the file has them
    want = _golden()[name]
    assert {k: v for k, v in got.items() if k != "steps"} == {k: v for k, v in want.items() if k != "steps"}
    for i, (g, w) in enumerate(zip(got["steps"], want["steps"])):
        assert g == w, f"step {i}"
    assert len(got["steps"]) == len(want["steps"]) == want["n_steps"]
