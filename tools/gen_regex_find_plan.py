#!/usr/bin/env python3
"""Planner figures of regex_find_clear / regex_starts_clear -> tests/golden/regex_find_plan.json.

The six patterns of tools/gen_regex_plan.py at 16 and 64 characters on uploaded strings, fused mode, whole DAGs (auto flush
off), rotation sharing as it is by default, the position (`find`) and the start flags (`starts`) each; and the wide position
once at 300 characters.  Per case: executed and extracted bootstraps, dependency levels, the level widths and the largest
sum c^2 any bootstrap input carries.  tests/test_regex_find.py pins the committed file; DESIGN section 25 quotes it.  No
GPU: a planner context records and levelises, nothing more.

    python tools/gen_regex_find_plan.py            # rewrite the file
    python tools/gen_regex_find_plan.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "regex_find_plan.json")
PATTERNS = (("abc", ""), ("error", ""), ("[A-Z]{2}-[0-9]+", ""), ("(error|warn).*timeout", "i"),
            (r"\w+@\w+\.(com|org)", ""), ("(ab|cd)*e?", ""))
SIZES = (16, 64)
CASES = tuple((call, p, f, n) for p, f in PATTERNS for n in SIZES for call in ("find", "starts"))
CASES += (("find_wide", "[A-Z]{2}-[0-9]+", "", 300),)
CALLS = {"find": "regex_find_clear", "starts": "regex_starts_clear", "find_wide": "regex_find_clear_wide"}


def key(call, pattern, flags, n):
    return "%s|%s|%s|%d" % (call, pattern, flags or "-", n)


def measure_find(call, pattern, flags, n):
    """flags: a string with `i` for ignore_case.  The figures of one call's flush on a fresh planner context."""
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        sk.set_mode(1)
        sk.set_auto_flush(0)
        s = sk.dummy_string(n)
        sk.flush()
        sk.stats(reset=True)
        keep = getattr(sk, CALLS[call])(s, pattern, ignore_case="i" in flags)
        sk.flush()
        st = sk.stats()
        widths = sk.level_widths()
        del keep
        return {"pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"], "levels": st["levels"],
                "level_widths": widths, "max_input_sum_c2": st["max_input_sum_c2"]}
    finally:
        sk.close()


def generate():
    return {"mode": "fused", "cases": {key(*c): measure_find(*c) for c in CASES}}


def main(argv):
    got = generate()
    if "--check" in argv:
        with open(PATH) as f:
            want = json.load(f)
        if got != want:
            print("regex_find_plan.json differs from what the planner records now")
            return 1
        print("regex_find_plan.json is up to date")
        return 0
    with open(PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, r in got["cases"].items():
        print("%-44s %6d bootstraps + %6d extracted, %3d levels, widest %5d, sum c^2 <= %d" % (
            name, r["pbs_executed"], r["pbs_extracted"], r["levels"], max(r["level_widths"], default=0), r["max_input_sum_c2"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
