#!/usr/bin/env python3
"""Planner figures of the wide (16-bit) string operations -> tests/golden/wide_plan.json.

For find_wide (encrypted four-character pattern) and len_wide on uploaded strings of 256, 1030 and 4097 characters, in
fused mode, whole DAGs (auto flush off), rotation sharing as it is by default: executed and extracted bootstraps,
dependency levels, the level widths and the largest sum c^2 any bootstrap input carries.  tests/test_wide_positions.py
pins the committed file; DESIGN section 15 quotes it.  No GPU: a planner context records and levelises, nothing more.

    python tools/gen_wide_plan.py            # rewrite the file
    python tools/gen_wide_plan.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "wide_plan.json")
SIZES = (256, 1030, 4097)
PATTERN_CHARS = 4


def measure(sk, op, n):
    """One operation on fresh uploaded inputs of a planner server key: the figures of its flush."""
    sk.set_mode(1)
    sk.set_auto_flush(0)
    s = sk.dummy_string(n)
    pat = sk.dummy_string(PATTERN_CHARS)
    sk.flush()
    sk.stats(reset=True)
    keep = sk.find_wide(s, pat) if op == "find_wide" else sk.len_wide(s)
    sk.flush()
    st = sk.stats()
    widths = sk.level_widths()
    del keep
    return {"pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"], "levels": st["levels"],
            "max_level_width": st["max_level_width"], "max_input_sum_c2": st["max_input_sum_c2"], "level_widths": widths}


def generate():
    from fhestring_amd.api import MyServerKey
    out = {"mode": "fused", "pattern_chars": PATTERN_CHARS, "ops": {}}
    for op in ("find_wide", "len_wide"):
        out["ops"][op] = {}
        for n in SIZES:
            sk = MyServerKey.planner()
            try:
                out["ops"][op][str(n)] = measure(sk, op, n)
            finally:
                sk.close()
    return out


def main(argv):
    got = generate()
    if "--check" in argv:
        with open(PATH) as f:
            want = json.load(f)
        if got != want:
            print("wide_plan.json differs from what the planner records now")
            return 1
        print("wide_plan.json is up to date")
        return 0
    with open(PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for op, per in got["ops"].items():
        for n, r in per.items():
            print("%-10s %5s chars: %6d bootstraps + %6d extracted, %2d levels, widest %5d" % (
                op, n, r["pbs_executed"], r["pbs_extracted"], r["levels"], r["max_level_width"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
