"""The string layer records what it recorded before its refactor (tests/golden/strings_digests.json,
tools/gen_strings_digests.py): on planner contexts (no GPU) every scenario's plan trace, the result's terms, the
statistics, the level widths and the launch groups hash to the committed digest.  Covers find / rfind / len / flag counts
in their u8 and wide forms at every shape that takes another branch, the digit boundaries of the fused forms, the limits
and the order of limit test and operand loading, char_at / substr / take / split_at with both kinds of position, constant
folding on trivial characters, every other string entry point of the C ABI once, and the pattern languages -- like_clear,
map_clear / class_flags / find_class, regex_clear, regex_find_clear / regex_starts_clear, with the user tables they apply
renamed by first appearance and hashed by content -- each in as-written and fused mode.
A digest that moves means that an entry point builds another DAG."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_strings_digests as gen  # noqa: E402

with open(gen.FIXTURE) as _f:
    GOLDEN = json.load(_f)


def test_fixture_lists_every_scenario():
    assert sorted(GOLDEN) == sorted(gen.SCENARIOS)


@pytest.mark.parametrize("name", sorted(gen.SCENARIOS))
def test_strings_digest(name):
    assert gen.SCENARIOS[name]() == GOLDEN[name], name
