#!/usr/bin/env python3
"""regex_clear on the MI355X next to contains_clear and like_clear, all legs in one process, f64-FFT arithmetic, fused mode.

    python tools/time_regex.py [--reps 10] [--out profiles/r20_regex.json] [--commit HASH] [--machine NAME]

On strings of 16 and 64 characters (text, one NUL of padding):
* a literal under search next to `contains_clear` of the same literal -- different DAGs: contains_clear is log-deep,
  regex_clear one level per character;
* a prefix pattern `lit.*` next to `like_clear('lit%')`;
* `[A-Z]{2}-[0-9]+` and `(error|warn).*timeout` with ignore_case;
* the last pattern over 16 strings, one fhs_submit each and one drain of all ticks, so that the 16 recurrences share their
  launch groups: the time per string next to the lone time.
One leg = record the operation + flush + stream sync on inputs that are already resident; medians of --reps after one
warm-up call.  Every leg's result is decrypted once, before the timing, against Python's `re`; every leg carries its
bootstrap counts (of all its strings) and levels (of one string), and its ms per level next to the narrow-level figure
contains_clear gives in the same run (its time over its levels).  No ratio is asserted: like_clear and contains_clear
are reference points, not bounds."""
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
BATCH = 16


def py_regex(buf, pattern, ignore_case=False, search=False):
    fn = re.search if search else re.fullmatch
    return int(fn(pattern.encode(), buf.split(b"\0")[0], re.S | (re.I if ignore_case else 0)) is not None)


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

    def leg(name, strings, want, op):
        """op on every string of `strings` (one: a plain flush; several: one submit each, then the drain)"""
        many = len(strings) > 1

        def once():
            out = []
            for s in strings:
                out.append(op(s))
                if many:
                    sk.submit()
            sk.flush()
            return out

        sk.flush()
        sk.stats(reset=True)
        got = [ck.decrypt_char(r) for r in once()]                   # warm-up, and the results
        st, widths = sk.stats(), sk.level_widths()
        assert got == [want] * len(strings), (name, got, want)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = once()
            del r
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        row = {"op": name, "chars": len(strings[0]), "strings": len(strings), "result": want, "ms_median": med,
               "ms_min": min(ts), "ms_max": max(ts), "spread": (max(ts) - min(ts)) / med, "ms_per_string": med / len(strings),
               "pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"], "levels": st["levels"] // len(strings),
               "ms_per_level": med * len(strings) / max(1, st["levels"]), "max_level_width": max(widths) if widths else 0,
               "max_input_sum_c2": st["max_input_sum_c2"]}
        res["legs"].append(row)
        print(json.dumps(row), flush=True)
        return row

    for n, text in sorted(TEXTS.items()):
        buf = text.encode() + bytes(1)
        assert len(buf) == n
        strings = [sk.upload_string(ck.encrypt_str_raw(text, 1)) for _ in range(BATCH)]
        s = strings[:1]
        lit, prefix = text[6:10], text[:5]
        base = leg("contains_clear(%r)" % lit, s, 1, lambda s: sk.contains_clear(s, lit))
        cases = [("regex_clear(%r, search)" % lit, lambda s: sk.regex_clear(s, re.escape(lit), search=True), 1),
                 ("like_clear(%r)" % (prefix + "%"), lambda s: sk.like_clear(s, prefix + "%"), 1),
                 ("regex_clear(%r)" % (prefix + ".*"), lambda s: sk.regex_clear(s, re.escape(prefix) + ".*"), 1),
                 ("regex_clear('[A-Z]{2}-[0-9]+')", lambda s: sk.regex_clear(s, "[A-Z]{2}-[0-9]+"),
                  py_regex(buf, "[A-Z]{2}-[0-9]+")),
                 ("regex_clear('(error|warn).*timeout', ignore_case, search)",
                  lambda s: sk.regex_clear(s, "(error|warn).*timeout", ignore_case=True, search=True),
                  py_regex(buf, "(error|warn).*timeout", True, True))]
        rows = [leg(name, s, want, op) for name, op, want in cases]
        name, op, want = cases[-1]
        batch = leg(name + " x %d, submit / pump" % BATCH, strings, want, op)
        batch["per_string_over_lone"] = batch["ms_per_string"] / rows[-1]["ms_median"]
        for row in rows + [batch]:
            row["ms_per_level_over_contains_clear"] = row["ms_per_level"] / base["ms_per_level"]
        del strings, s
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
