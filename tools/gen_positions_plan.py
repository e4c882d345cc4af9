#!/usr/bin/env python3
"""Planner figures of the operations that consume an encrypted position -> tests/golden/positions_plan.json.

char_at, substr (count = n and count = 8), take and split_at on uploaded strings of 64, 256 and 512 characters with an
uploaded u8 position, and char_at_wide and substr_wide (count = 8) on 1030 and 4097 characters with an uploaded wide
position, in fused mode, whole DAGs (auto flush off), rotation sharing as it is by default: executed and extracted
bootstraps, dependency levels, the level widths and the largest sum c^2 any bootstrap input carries.
tests/test_positions.py pins the committed file; DESIGN section 19 quotes it.  No GPU: a planner context records and
levelises, nothing more.

    python tools/gen_positions_plan.py            # rewrite the file
    python tools/gen_positions_plan.py --check    # compare, exit 1 on a difference
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "positions_plan.json")
NARROW_SIZES = (64, 256, 512)
WIDE_SIZES = (1030, 4097)
NARROW_OPS = ("char_at", "substr_n", "substr_8", "take", "split_at")
WIDE_OPS = ("char_at_wide", "substr_wide_8")


def run_op(sk, op, s, pos):
    """The operation `op` names, on a string and a position of the matching width."""
    n = len(s)
    if op in ("char_at", "char_at_wide"):
        return sk.char_at(s, pos)
    if op in ("substr_8", "substr_wide_8"):
        return sk.substr(s, pos, 8)
    if op == "substr_n":
        return sk.substr(s, pos, n)
    if op == "take":
        return sk.take(s, pos)
    if op == "split_at":
        return sk.split_at(s, pos)
    raise ValueError(op)


def measure(sk, op, n):
    """One operation on fresh uploaded inputs of a planner server key: the figures of its flush."""
    from fhestring_amd.api import FheU16
    sk.set_mode(1)
    sk.set_auto_flush(0)
    s = sk.dummy_string(n)
    p = sk.dummy_string(2)
    pos = FheU16(p[0], p[1]) if op.endswith("_wide") or "_wide_" in op else p[0]
    sk.flush()
    sk.stats(reset=True)
    keep = run_op(sk, op, s, pos)
    sk.flush()
    st = sk.stats()
    widths = sk.level_widths()
    del keep
    return {"pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"], "levels": st["levels"],
            "max_level_width": st["max_level_width"], "max_input_sum_c2": st["max_input_sum_c2"], "level_widths": widths}


def generate():
    from fhestring_amd.api import MyServerKey
    out = {"mode": "fused", "ops": {}}
    for ops, sizes in ((NARROW_OPS, NARROW_SIZES), (WIDE_OPS, WIDE_SIZES)):
        for op in ops:
            out["ops"][op] = {}
            for n in sizes:
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
            print("positions_plan.json differs from what the planner records now")
            return 1
        print("positions_plan.json is up to date")
        return 0
    with open(PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for op, per in got["ops"].items():
        for n, r in per.items():
            print("%-14s %5s chars: %6d bootstraps + %6d extracted, %2d levels, widest %5d, sum c^2 <= %d" % (
                op, n, r["pbs_executed"], r["pbs_extracted"], r["levels"], r["max_level_width"], r["max_input_sum_c2"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
