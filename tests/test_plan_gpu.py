"""The cut of a frame is the recorded one, case by case (tests/golden/plan_usage.json, written by
scripts/plan_usage.py at the commit before the pass planner moved to rt_plan.cpp): streams,
workspaces, pass sizes, workspace bytes, pair and split passes, the deep launch and the tile classes
as rt_scene_usage_get reports them after a render. The bit-exact tests cannot see a plan that
changed (the bits never depend on the cut); this one can.

The cases and the way each is rendered come from the fixture and from the recorder's own
run_case(), so the record and the replay cannot drift apart.
"""
import importlib.util
import json
import os
import time

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_SECONDS = 5.0  # a case is one scene and one or two frames of at most 70 x 37 x 96 samples: a fraction of a second


def _recorder():
    spec = importlib.util.spec_from_file_location("plan_usage", os.path.join(REPO, "scripts", "plan_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_recorded_plan_is_unchanged():
    """Every case of the fixture, in order, field by field. A case that raises (a HIP error
    surfaces as RtError) ends the test there: no later case runs on a device in that state.
    CASE_SECONDS is checked when a case returns, so a slow case fails the test before the next one
    starts; it cannot end a case that never returns (that is left to the runner's own time limit)."""
    rec = _recorder()
    with open(os.path.join(REPO, "tests", "golden", "plan_usage.json")) as f:
        fixture = json.load(f)
    assert tuple(fixture["fields"]) == rec.FIELDS
    # the fixture holds the recorder's case list (a case added to one and not the other is an error)
    assert [{k: v for k, v in c.items() if k != "usage"} for c in fixture["cases"]] == rec.case_list()
    assert len(fixture["cases"]) >= 40
    for case in fixture["cases"]:
        t0 = time.perf_counter()
        got = rec.run_case(case)
        took = time.perf_counter() - t0
        assert took < CASE_SECONDS, f"{case['name']}: {took:.1f} s"
        want = case["usage"]
        diff = {k: (got[k], want[k]) for k in rec.FIELDS if got[k] != want[k]}
        assert not diff, f"{case['name']}: (got, recorded) {diff}"
