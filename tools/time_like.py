#!/usr/bin/env python3
"""like_clear on the MI355X next to contains_clear, all legs in one process, f64-FFT arithmetic, fused mode.

    python tools/time_like.py [--reps 10] [--out profiles/r18_like.json] [--commit HASH] [--machine NAME]

On strings of 64 and 256 characters (text, one NUL of padding):
* `contains_clear(lit)` and `like_clear('%lit%')`: one DAG, so their ratio is the run-to-run spread; `spread` of a leg is
  (max - min) / median of its repeats, and the two medians are expected inside each other's;
* `like_clear` with 1, 2 and 4 middle segments between an anchored first and last one (`a%b%c` shapes), one ignore_case
  pattern, one pattern with `_` and an end anchor: written down as measured, next to contains_clear of the same run.
One leg = record the operation + flush + stream sync on inputs that are already resident; medians of --reps after one
warm-up call.  Every leg's result is decrypted once, before the timing, against Python's `re`; every leg carries its
bootstrap counts and level widths."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:
    import torch  # noqa: F401  (one HIP runtime in the process: torch first, like bench.py)
except ImportError:
    pass

from fhestring_amd.api import MyClientKey, MyServerKey  # noqa: E402

LIT = "Qz7#x"
FILLER = "abcdefghijklmnopqrstuvwxy" * 11


def py_like(buf, pattern, ignore_case=False):
    body = b"".join(rb"[\x00-\xff]*" if c == "%" else rb"[^\x00]" if c == "_" else re.escape(c.encode()) for c in pattern)
    return int(re.match(rb"\A" + body + rb"(?=\x00|\Z)", buf, re.S | (re.I if ignore_case else 0)) is not None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="")
    ap.add_argument("--machine", default="")
    a = ap.parse_args()
    ck = MyClientKey(0x71DE)
    sk = MyServerKey.from_client_key(ck, arith=1)
    sk.set_mode(1)
    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "arith": "f64_fft", "legs": []}

    def leg(name, s, want, op):
        sk.flush()
        sk.stats(reset=True)
        got = ck.decrypt_char(op(s))                                  # warm-up, and the result
        st, widths = sk.stats(), sk.level_widths()
        assert got == want, (name, len(s), got, want)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = op(s)
            sk.flush()
            del r
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        row = {"op": name, "chars": len(s), "result": got, "ms_median": med, "ms_min": min(ts), "ms_max": max(ts),
               "spread": (max(ts) - min(ts)) / med, "pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"],
               "levels": st["levels"], "level_widths": widths, "max_input_sum_c2": st["max_input_sum_c2"]}
        res["legs"].append(row)
        print(json.dumps(row), flush=True)
        return row

    for n in (64, 256):
        at = n - 12
        text = FILLER[:at] + LIT + FILLER[at + len(LIT):n - 1]
        buf = text.encode() + bytes(1)
        assert len(buf) == n and text.find(LIT) == at
        s = sk.upload_string(ck.encrypt_str_raw(text, 1))
        base = leg("contains_clear(%r)" % LIT, s, 1, lambda s: sk.contains_clear(s, LIT))
        patterns = [("%" + LIT + "%", False),
                    ("abc%" + LIT + "%" + text[-2:], False),                                   # 1 middle segment
                    ("abc%klm%" + LIT + "%" + text[-2:], False),                               # 2
                    ("abc%fgh%klm%" + LIT[:2] + "%" + LIT[2:] + "%" + text[-2:], False),       # 4
                    ("%" + LIT.swapcase() + "%", True),
                    ("%" + LIT[:2] + "_" + LIT[3:] + "_" * (n - 1 - at - len(LIT)), False)]     # `_`, and the end anchor
        for pattern, ic in patterns:
            row = leg("like_clear(%r%s)" % (pattern, ", ignore_case" if ic else ""), s, py_like(buf, pattern, ic),
                      lambda s: sk.like_clear(s, pattern, ignore_case=ic))
            assert row["result"] == 1, pattern
            row["over_contains_clear"] = row["ms_median"] / base["ms_median"]
        infix = res["legs"][-len(patterns)]
        assert (infix["pbs_executed"], infix["level_widths"]) == (base["pbs_executed"], base["level_widths"])
        res["infix_over_contains_%d" % n] = infix["ms_median"] / base["ms_median"]
        res["infix_within_spread_%d" % n] = bool(abs(infix["ms_median"] - base["ms_median"]) <=
                                                 max(infix["spread"] * infix["ms_median"], base["spread"] * base["ms_median"]))
        del s
    sk.close()
    ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}))


if __name__ == "__main__":
    main()
