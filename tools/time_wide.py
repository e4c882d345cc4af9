#!/usr/bin/env python3
"""The wide (16-bit) string operations on the MI355X, all legs in one process, f64-FFT arithmetic, fused mode.

    python tools/time_wide.py [--reps 10] [--out profiles/r12_wide.json] [--commit HASH] [--machine NAME]

* `find` and `find_wide` on config 3's input (256 characters + NUL, encrypted four-character pattern): below 256 windows
  the two record the same bootstraps in the same levels (digits 4 to 7 are linear), so their ratio is the run-to-run
  spread of one DAG; it is written down, not asserted.
* `find_clear_wide`, `find_wide` and `len_wide` at 1024 and 4097 characters.
One leg = record the operation + flush + stream sync on inputs that are already resident; medians of --reps after one
warm-up call.  Every leg's result is decrypted once, before the timing."""
import argparse
import json
import os
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

PAT = "Qz7#"


def med(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3, min(ts) * 1e3


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
    filler = "abcdefghijklmnopqrstuvwxy" * 164
    pat = sk.upload_string(ck.encrypt_str_raw(PAT, 0))
    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "arith": "f64_fft", "legs": []}

    def leg(name, n, pos, op, decrypt):
        text = filler[:pos] + PAT + filler[pos + len(PAT):n]
        s = sk.upload_string(ck.encrypt_str_raw(text, 1))
        sk.stats(reset=True)
        got = decrypt(op(s))                                          # warm-up, and the result
        st = sk.stats()
        want = n if name.startswith("len") else pos
        assert got == want, (name, n, got, want)

        def once():
            r = op(s)
            sk.flush()
            del r

        t = med(once, a.reps)
        row = {"op": name, "chars": n, "match_at": pos, "ms_median": t[0], "ms_min": t[1], "pbs_executed": st["pbs_executed"],
               "pbs_extracted": st["pbs_extracted"], "levels": st["levels"], "max_input_sum_c2": st["max_input_sum_c2"]}
        res["legs"].append(row)
        print(json.dumps(row), flush=True)
        return row

    u8 = leg("find", 256, 201, lambda s: sk.find(s, pat), ck.decrypt_char)
    wide = leg("find_wide", 256, 201, lambda s: sk.find_wide(s, pat), ck.decrypt_u16)
    res["find_wide_over_find_256"] = wide["ms_median"] / u8["ms_median"]
    for n in (1024, 4097):
        leg("find_clear_wide", n, n - 5, lambda s: sk.find_clear_wide(s, PAT), ck.decrypt_u16)
        leg("find_wide", n, n - 5, lambda s: sk.find_wide(s, pat), ck.decrypt_u16)
        leg("len_wide", n, n - 5, lambda s: sk.len_wide(s), ck.decrypt_u16)
    sk.close()
    ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
