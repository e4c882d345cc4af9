#!/usr/bin/env python3
"""regex_find_clear on the MI355X next to regex_clear(search=True) and find_clear, all legs in one process, f64-FFT
arithmetic, fused mode.

    python tools/time_regex_find.py [--reps 10] [--out profiles/r23_regex_find.json] [--commit HASH] [--machine NAME]

On strings of 16 and 64 characters (text, one NUL of padding), per pattern -- a literal, `[A-Z]{2}-[0-9]+`, and
`(error|warn).*timeout` with ignore_case -- the position (regex_find_clear) next to the flag of the same pattern
(regex_clear under search); for the literal also find_clear, the log-deep DAG of the same question.
One leg = record the operation + flush + stream sync on inputs that are already resident; medians of --reps after one
warm-up call, whose result is decrypted against Python's `re`.  Every leg carries its bootstrap, extraction and level
counts and its ms per level; a regex_find_clear leg also that figure over regex_clear's of the same pattern in the same
run -- the comparison DESIGN section 25 writes down.  Nothing is asserted about the times."""
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

TEXTS = {16: "warn: a timeout", 64: "AB-2024 Error: the request to host 7 ran into a TIMEOUT again".ljust(63, ".")}


def rx(pattern, ignore_case=False):
    return re.compile(pattern.encode(), re.S | (re.I if ignore_case else 0))


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
        def once():
            r = op(s)
            sk.flush()
            return r

        sk.flush()
        sk.stats(reset=True)
        got = ck.decrypt_char(once())                        # warm-up, and the result
        st, widths = sk.stats(), sk.level_widths()
        assert got == want, (name, got, want)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = once()
            del r
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        row = {"op": name, "chars": len(s), "result": want, "ms_median": med, "ms_min": min(ts), "ms_max": max(ts),
               "spread": (max(ts) - min(ts)) / med, "pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"],
               "levels": st["levels"], "ms_per_level": med / max(1, st["levels"]),
               "max_level_width": max(widths) if widths else 0, "max_input_sum_c2": st["max_input_sum_c2"]}
        res["legs"].append(row)
        print(json.dumps(row), flush=True)
        return row

    for n, text in sorted(TEXTS.items()):
        buf = text.encode() + bytes(1)
        assert len(buf) == n
        s = sk.upload_string(ck.encrypt_str_raw(text, 1))
        lit = text[6:10]
        for pattern, kw in ((re.escape(lit), {}), ("[A-Z]{2}-[0-9]+", {}), ("(error|warn).*timeout", {"ignore_case": True})):
            m = rx(pattern, **kw).search(text.encode())
            flag = leg("regex_clear(%r, search%s)" % (pattern, ", ignore_case" if kw else ""), s, int(m is not None),
                       lambda s: sk.regex_clear(s, pattern, search=True, **kw))
            find = leg("regex_find_clear(%r%s)" % (pattern, ", ignore_case" if kw else ""), s, m.start() if m else 255,
                       lambda s: sk.regex_find_clear(s, pattern, **kw))
            find["ms_per_level_over_regex_clear"] = find["ms_per_level"] / flag["ms_per_level"]
            if pattern == re.escape(lit):
                leg("find_clear(%r)" % lit, s, text.find(lit), lambda s: sk.find_clear(s, lit))
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
