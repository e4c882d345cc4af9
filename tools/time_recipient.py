#!/usr/bin/env python3
"""Packed download under a recipient's key on the MI355X: `download_packed` of 64 / 1024 / 4097-character strings under
the context's own key, the way the parent commit does it, beside `download_packed(recipient=True)` and, for scale, beside an
in-place `store_rekey` of an entry of the same size, all in one process.

    python tools/time_recipient.py [--reps 10] [--out FILE.json] [--commit HASH] [--machine NAME]

Both downloads end with a stream wait of their own; re-key = host call + stream sync (tools/time_rekey.py).  The recipient
form runs one launch of rekey_packed_kernel per pass of up to four groups in place of pack_switch16_kernel, so the one
criterion is
    recipient download <= own-key download + 2 x passes x (the same run's in-place re-key)
with the factor 2 for the 512 B-per-instruction u64 loads and the 2-byte stores the 32-bit kernel does not have.  It is
written down, not tuned: the exit status says whether it held.  Before the timing the recipient's words are decrypted once
with the second client's key."""
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
    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "recipient": []}
    for n in (64, 1024, 4097):
        t = text(n - 1)
        s = sk.upload_compressed_string(ca.encrypt_compressed(t, 1))
        e = sk.store_put(s)
        assert ca.decrypt_packed(sk.download_packed(s)) == t                         # warm-up, and the results
        assert cb.decrypt_packed(sk.download_packed(s, recipient=True)) == t

        def in_place():
            e.rekey()
            sk.stream_sync()

        in_place()
        t_own = med(lambda: sk.download_packed(s), a.reps)
        t_rec = med(lambda: sk.download_packed(s, recipient=True), a.reps)
        t_own2 = med(lambda: sk.download_packed(s), a.reps)                          # again: drift inside the run
        t_in = med(in_place, a.reps)
        groups = (4 * n + 2047) // 2048
        passes = (groups + 3) // 4
        row = {"chars": n, "groups": groups, "passes": passes,
               "own_key_ms_median": t_own[0], "own_key_ms_min": t_own[1],
               "own_key_again_ms_median": t_own2[0], "own_key_again_ms_min": t_own2[1],
               "recipient_ms_median": t_rec[0], "recipient_ms_min": t_rec[1],
               "rekey_in_place_ms_median": t_in[0], "rekey_in_place_ms_min": t_in[1],
               "added_per_pass_ms": (t_rec[0] - t_own[0]) / passes,
               "allowed_per_pass_ms": 2 * t_in[0],
               "criterion": bool(t_rec[0] <= t_own[0] + 2 * passes * t_in[0])}
        res["recipient"].append(row)
        print(json.dumps(row), flush=True)
        e.drop()
        del s
    res["criterion_recipient_within_two_rekeys_per_pass"] = all(r["criterion"] for r in res["recipient"])
    sk.close()
    for ck in (ca, cb):
        ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["criterion_recipient_within_two_rekeys_per_pass"]:
        sys.exit("the recipient download costs more than two in-place re-keys per pass over the own-key download")


if __name__ == "__main__":
    main()
