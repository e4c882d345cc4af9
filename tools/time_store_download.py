#!/usr/bin/env python3
"""Packed download of parked store entries on the MI355X: `StoredString.download_packed` of 64 / 1024 / 4097-character
entries under the entry's own key and for a recipient, a 64-character window of the 4097-character entry, and beside each
the only route the parent commit has for the same characters -- `get` + `download_packed[_for]` + release of the handles
-- all in one process.

    python tools/time_store_download.py [--reps 10] [--out FILE.json] [--commit HASH] [--machine NAME]

Every leg ends with a stream wait of its own (the download's).  Medians of `reps` after a warm-up of every leg.  The route
through the handles contains the same device-to-host copy plus the expansion and the eleven levels of the packing tree, so
the one criterion, at every size, for the window and under both keys, is
    direct download < get + packed download of the same characters, in the same run
without a margin.  It is written down, not tuned: the exit status says whether it held.  Before the timing both forms are
decrypted once, with the first and the second client's key."""
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
import numpy as np  # noqa: E402

from fhestring_amd.api import MyClientKey, MyServerKey  # noqa: E402


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
    ca, cb = MyClientKey(0x7135), MyClientKey(0x7136)
    sk = MyServerKey.from_client_key(ca, arith=1)
    sk.set_mode(1)
    sk.load_packing_key(ca)
    sk.load_rekey_key(ca.rekey_key(cb))
    rng = np.random.default_rng(1)
    text = lambda n: "".join(chr(v) for v in rng.integers(97, 123, n))
    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "store_download": []}

    def legs(e, t, first, count, what):
        want = t[first:first + count]

        def through_handles(recipient):
            s = e.get(first, count)
            p = sk.download_packed(s, recipient=recipient)
            del s                                                    # releases the pool blocks
            return p

        assert ca.decrypt_packed(e.download_packed(first, count)) == want          # warm-up, and the results
        assert cb.decrypt_packed(e.download_packed(first, count, recipient=True)) == want
        assert ca.decrypt_packed(through_handles(False)) == want
        assert cb.decrypt_packed(through_handles(True)) == want
        t_own = med(lambda: e.download_packed(first, count), a.reps)
        t_rec = med(lambda: e.download_packed(first, count, recipient=True), a.reps)
        t_old = med(lambda: through_handles(False), a.reps)
        t_old_rec = med(lambda: through_handles(True), a.reps)
        t_own2 = med(lambda: e.download_packed(first, count), a.reps)              # again: drift inside the run
        row = {"leg": what, "entry_chars": len(e), "first_char": first, "chars": count,
               "bytes_over_the_bus": int(e.download_packed(first, count).nbytes - 16),
               "direct_ms_median": t_own[0], "direct_ms_min": t_own[1],
               "direct_again_ms_median": t_own2[0], "direct_again_ms_min": t_own2[1],
               "direct_recipient_ms_median": t_rec[0], "direct_recipient_ms_min": t_rec[1],
               "get_download_release_ms_median": t_old[0], "get_download_release_ms_min": t_old[1],
               "get_download_for_release_ms_median": t_old_rec[0], "get_download_for_release_ms_min": t_old_rec[1],
               "criterion_own_key": bool(t_own[0] < t_old[0]), "criterion_recipient": bool(t_rec[0] < t_old_rec[0])}
        res["store_download"].append(row)
        print(json.dumps(row), flush=True)

    for n in (64, 1024, 4097):
        t = text(n - 1)
        s = sk.upload_compressed_string(ca.encrypt_compressed(t, 1))
        e = sk.store_put(s)
        del s
        legs(e, t, 0, n, "whole entry")
        if n == 4097:
            legs(e, t, 2000, 64, "window")                           # straddles groups 3 | 4, first_coef 1856
        e.drop()
    res["criterion_direct_faster_than_through_handles"] = all(r["criterion_own_key"] and r["criterion_recipient"]
                                                              for r in res["store_download"])
    sk.close()
    for ck in (ca, cb):
        ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["criterion_direct_faster_than_through_handles"]:
        sys.exit("a direct download of a parked entry was not faster than get + packed download of the same characters")


if __name__ == "__main__":
    main()
