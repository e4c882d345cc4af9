#!/usr/bin/env python3
"""Planner figures of regex_clear -> tests/golden/regex_plan.json.

Six (pattern, flags) cases at 16 and 64 characters on uploaded strings, fused mode, whole DAGs (auto flush off), rotation
sharing as it is by default: executed and extracted bootstraps, dependency levels, the level widths and the largest
sum c^2 any bootstrap input carries.  tests/test_regex.py pins the committed file; DESIGN section 22 quotes it.  No GPU: a
planner context records and levelises, nothing more.

    python tools/gen_regex_plan.py            # rewrite the file
    python tools/gen_regex_plan.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_like_plan import measure  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "regex_plan.json")
PATTERNS = (("abc", ""), ("error", "s"), ("[A-Z]{2}-[0-9]+", ""), ("(error|warn).*timeout", "i"),
            (r"\w+@\w+\.(com|org)", ""), ("(ab|cd)*e?", ""))
SIZES = (16, 64)
CASES = tuple((p, f, n) for p, f in PATTERNS for n in SIZES)


def key(pattern, flags, n):
    return "%s|%s|%d" % (pattern, flags or "-", n)


def measure_regex(pattern, flags, n):
    """flags: a string with `i` for ignore_case and `s` for search"""
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        return measure(sk, lambda sk, s: sk.regex_clear(s, pattern, ignore_case="i" in flags, search="s" in flags), n)
    finally:
        sk.close()


def generate():
    return {"mode": "fused", "cases": {key(*c): measure_regex(*c) for c in CASES}}


def main(argv):
    got = generate()
    if "--check" in argv:
        with open(PATH) as f:
            want = json.load(f)
        if got != want:
            print("regex_plan.json differs from what the planner records now")
            return 1
        print("regex_plan.json is up to date")
        return 0
    with open(PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, r in got["cases"].items():
        print("%-34s %6d bootstraps + %6d extracted, %2d levels, widest %5d, sum c^2 <= %d" % (
            name, r["pbs_executed"], r["pbs_extracted"], r["levels"], r["max_level_width"], r["max_input_sum_c2"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
