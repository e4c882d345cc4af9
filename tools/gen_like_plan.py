#!/usr/bin/env python3
"""Planner figures of like_clear -> tests/golden/like_plan.json.

Six (pattern, ignore_case, characters) cases on uploaded strings, fused mode, whole DAGs (auto flush off), rotation sharing
as it is by default: executed and extracted bootstraps, dependency levels, the level widths and the largest sum c^2 any
bootstrap input carries.  tests/test_like.py pins the committed file; DESIGN section 20 quotes it.  No GPU: a planner
context records and levelises, nothing more.

    python tools/gen_like_plan.py            # rewrite the file
    python tools/gen_like_plan.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "like_plan.json")
CASES = (("%ma%", False, 64), ("%hello%", False, 256), ("INV-2024-%", False, 64), ("%@example.___", False, 64),
         ("a%b%c", False, 64), ("%error%timeout%", True, 256))


def key(pattern, ignore_case, n):
    return "%s|%s|%d" % (pattern, "ilike" if ignore_case else "like", n)


def measure(sk, op, n):
    """op(sk, s) on a fresh uploaded string of n characters of a planner server key: the figures of its flush."""
    sk.set_mode(1)
    sk.set_auto_flush(0)
    s = sk.dummy_string(n)
    sk.flush()
    sk.stats(reset=True)
    keep = op(sk, s)
    sk.flush()
    st = sk.stats()
    widths = sk.level_widths()
    figure = keep.sum_c2()
    del keep
    return {"pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"], "levels": st["levels"],
            "max_level_width": st["max_level_width"], "max_input_sum_c2": st["max_input_sum_c2"], "level_widths": widths,
            "result_sum_c2": figure}


def measure_like(pattern, ignore_case, n, escape=None):
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        return measure(sk, lambda sk, s: sk.like_clear(s, pattern, escape=escape, ignore_case=ignore_case), n)
    finally:
        sk.close()


def generate():
    return {"mode": "fused", "cases": {key(*c): measure_like(*c) for c in CASES}}


def main(argv):
    got = generate()
    if "--check" in argv:
        with open(PATH) as f:
            want = json.load(f)
        if got != want:
            print("like_plan.json differs from what the planner records now")
            return 1
        print("like_plan.json is up to date")
        return 0
    with open(PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, r in got["cases"].items():
        print("%-28s %6d bootstraps + %6d extracted, %2d levels, widest %5d, sum c^2 <= %d" % (
            name, r["pbs_executed"], r["pbs_extracted"], r["levels"], r["max_level_width"], r["max_input_sum_c2"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
