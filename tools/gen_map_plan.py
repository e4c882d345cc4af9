#!/usr/bin/env python3
"""Planner figures of map_clear and class_flags -> tests/golden/map_plan.json.

The named tables and classes of DESIGN section 21 on uploaded strings of 16 and 64 characters, fused mode, whole DAGs
(auto flush off): executed and extracted bootstraps, dependency levels, the largest sum c^2 any bootstrap input carries
and the noise figure of the result.  tests/test_map.py pins the committed file and takes its tables and classes from
here.  No GPU: a planner context records and levelises, nothing more.

    python tools/gen_map_plan.py            # rewrite the file
    python tools/gen_map_plan.py --check    # compare, exit 1 on a difference
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "map_plan.json")
SIZES = (16, 64)

_RNG = random.Random(0x7AB1E)
IDENTITY = bytes(range(256))
LETTERS = b"abcdefghijklmnopqrstuvwxyz"
TABLES = {
    "identity": IDENTITY,
    "constant": b"*" * 256,
    "to_upper": bytes(v - 32 if 0x61 <= v <= 0x7A else v for v in range(256)),
    "to_lower": bytes(v + 32 if 0x41 <= v <= 0x5A else v for v in range(256)),
    "mask_digits": bytes.maketrans(b"0123456789", b"#" * 10),
    "rot13": bytes.maketrans(LETTERS + LETTERS.upper(), LETTERS[13:] + LETTERS[:13] + LETTERS[13:].upper() + LETTERS[:13].upper()),
    "bit_reversal": bytes(int("{:08b}".format(v)[::-1], 2) for v in range(256)),
    "random": bytes(_RNG.randrange(256) for _ in range(256)),
}
CLASSES = {
    "digits": "0-9",
    "lower": "a-z",
    "letters": "A-Za-z",
    "hex": "0-9A-Fa-f",
    "identifier": "A-Za-z0-9_",
    "whitespace": b" \t\n\r\x0b\x0c",
    "empty": b"",
    "full": bytes(range(256)),
}


def measure(op, n):
    """op(sk, s) -> FheString on a fresh uploaded string of n characters of a planner server key: the figures of its flush"""
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        sk.set_mode(1)
        sk.set_auto_flush(0)
        s = sk.dummy_string(n)
        sk.flush()
        sk.stats(reset=True)
        keep = op(sk, s)
        sk.flush()
        st = sk.stats()
        figure = max(c.sum_c2() for c in keep)
        del keep
        return {"pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"], "levels": st["levels"],
                "max_input_sum_c2": st["max_input_sum_c2"], "result_sum_c2": figure}
    finally:
        sk.close()


def measure_map(name, n):
    return measure(lambda sk, s: sk.map_clear(s, TABLES[name]), n)


def measure_class(name, n):
    return measure(lambda sk, s: sk.class_flags(s, CLASSES[name]), n)


def generate():
    out = {"mode": "fused", "map_clear": {}, "class_flags": {}}
    for n in SIZES:
        for name in TABLES:
            out["map_clear"]["%s|%d" % (name, n)] = measure_map(name, n)
        for name in CLASSES:
            out["class_flags"]["%s|%d" % (name, n)] = measure_class(name, n)
    return out


def main(argv):
    got = generate()
    if "--check" in argv:
        with open(PATH) as f:
            want = json.load(f)
        if got != want:
            print("map_plan.json differs from what the planner records now")
            return 1
        print("map_plan.json is up to date")
        return 0
    with open(PATH, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for kind in ("map_clear", "class_flags"):
        for name, r in got[kind].items():
            print("%-12s %-18s %6d bootstraps + %4d extracted, %d levels, sum c^2 <= %2d, result %d" % (
                kind, name, r["pbs_executed"], r["pbs_extracted"], r["levels"], r["max_input_sum_c2"], r["result_sum_c2"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
