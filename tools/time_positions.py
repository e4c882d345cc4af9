#!/usr/bin/env python3
"""The consumers of encrypted positions on the MI355X, all legs in one process, f64-FFT arithmetic, fused mode.

    python tools/time_positions.py [--reps 10] [--out profiles/r16_positions.json] [--commit HASH] [--machine NAME]

* `find_clear` alone against `find_clear` + `substr(count=8)` in one DAG on 64 and 256 characters: what using the
  position on the server adds to finding it.
* `char_at`, `take` and `split_at` on 256 characters, the position find_clear's.
* `find_clear_wide` + `substr_wide(count=8)` on 1030 and 4097 characters.
One leg = record the operations + flush + stream sync on inputs that are already resident; medians of --reps after one
warm-up call.  Every leg's result is decrypted once, before the timing.  Nothing is asserted about the times: they are
written down beside the planner's bootstrap and level counts (DESIGN section 19 projects about eight 1024-row rounds
plus the bit level for substr(count=n) on 256 characters from section 7's rates)."""
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
    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "arith": "f64_fft", "legs": []}

    def plain(chars):
        return bytes(ck.decrypt_char_raw(row) for row in chars.download())

    def leg(name, n, pos, op, check):
        """op(s) -> result; check(result, text) asserts it once, on the warm-up call"""
        text = filler[:pos] + PAT + filler[pos + len(PAT):n - 1]
        s = sk.upload_string(ck.encrypt_str_raw(text, 1))
        assert len(s) == n
        sk.stats(reset=True)
        check(op(s), text.encode() + b"\0")
        st = sk.stats()

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

    def is_pos(wide):
        dec = ck.decrypt_u16 if wide else ck.decrypt_char
        return lambda r, buf: _eq(dec(r), buf.find(PAT.encode()))

    def _eq(got, want):
        assert got == want, (got, want)

    def is_sub8(r, buf):
        p = buf.find(PAT.encode())
        _eq(plain(r), (buf[p:p + 8] + bytes(8))[:8])

    for n in (64, 256):
        pos = n - 30
        alone = leg("find_clear", n, pos, lambda s: sk.find_clear(s, PAT), is_pos(False))
        both = leg("find_clear+substr_8", n, pos, lambda s: sk.substr(s, sk.find_clear(s, PAT), 8), is_sub8)
        res["substr_8_over_find_clear_%d" % n] = both["ms_median"] / alone["ms_median"]
    n, pos = 256, 201
    leg("find_clear+char_at", n, pos, lambda s: sk.char_at(s, sk.find_clear(s, PAT)),
        lambda r, buf: _eq(ck.decrypt_char(r), ord(PAT[0])))
    leg("find_clear+take", n, pos, lambda s: sk.take(s, sk.find_clear(s, PAT)),
        lambda r, buf: _eq(plain(r), buf[:pos] + bytes(n - pos)))
    leg("find_clear+split_at", n, pos, lambda s: sk.split_at(s, sk.find_clear(s, PAT)),
        lambda r, buf: _eq((plain(r[0]), plain(r[1])), (buf[:pos] + bytes(n - pos), buf[pos:] + bytes(pos))))
    for n in (1030, 4097):
        leg("find_clear_wide", n, n - 30, lambda s: sk.find_clear_wide(s, PAT), is_pos(True))
        leg("find_clear_wide+substr_wide_8", n, n - 30, lambda s: sk.substr(s, sk.find_clear_wide(s, PAT), 8), is_sub8)
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
