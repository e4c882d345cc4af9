"""The host planner reproduces the committed plan digests (tests/golden/plan_digests.json, tools/gen_plan_digests.py): on
planner contexts (no GPU) every scenario's plan trace -- the rows of every launch group in order, the shared extractions,
the group ends -- the result's terms, the statistics, the level widths and the launch groups hash to what was recorded.
Covers rotation sharing on and off, round alignment, the automatic partial flush (the 8 192-rotation peel), submit /
pump scheduling, as-written mode, the compressed and public uploads, and the fhs_flush_plan / _level_exec /
_level_commit walk of two ranks.  A digest that moves is a change of the engine's behaviour."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_plan_digests as gen  # noqa: E402

with open(gen.FIXTURE) as _f:
    GOLDEN = json.load(_f)


def test_fixture_lists_every_scenario():
    assert sorted(GOLDEN) == sorted(gen.SCENARIOS)


@pytest.mark.parametrize("name", sorted(gen.SCENARIOS))
def test_plan_digest(name):
    assert gen.SCENARIOS[name]() == GOLDEN[name], name
