#!/usr/bin/env python3
"""String store re-key on the MI355X: fhs_store_rekey of 64 / 1024 / 4097-character entries, in place and as a copy, beside
what has to happen without it -- the round trip through the secret-key holder -- and beside `put` alone, all in one process.

    python tools/time_rekey.py [--reps 10] [--out FILE.json] [--commit HASH] [--machine NAME]

re-key = host call + stream sync (the call only enqueues its one launch).  Repeated re-keys of one entry with the same key
turn its contents into noise; the kernel's work does not depend on the words, and the result is checked once, before the
timing, by decrypting an export with the second client's key.  The copy leg includes the allocation of the new entry and
its release.
round trip = get + packed download + client decryption (client a) + compressed encryption (client b) + upload + put on a
second context under b's keys, everything the parent commit needs to move one parked string from key a to key b.
put = the last step of that alone.  The one criterion: the re-key of the 4097-character entry is faster than the same
run's put of it (put runs eleven tree levels of the node arithmetic the re-key runs once)."""
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
    ska, skb = MyServerKey.from_client_key(ca, arith=1), MyServerKey.from_client_key(cb, arith=1)
    for sk, ck in ((ska, ca), (skb, cb)):
        sk.set_mode(1)
        sk.load_packing_key(ck)
    ska.load_rekey_key(ca.rekey_key(cb))
    rng = np.random.default_rng(1)
    text = lambda n: "".join(chr(v) for v in rng.integers(97, 123, n))
    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "rekey": []}
    for n in (64, 1024, 4097):
        t = text(n - 1)
        s = ska.upload_compressed_string(ca.encrypt_compressed(t, 1))
        e = ska.store_put(s)
        del s
        moved = e.rekey(copy=True)                                   # warm-up, and the result under b's key
        assert cb.decrypt_str_raw(moved.export()[0].expand()) == t and ca.decrypt(e.get()) == t
        moved.drop()

        def in_place():
            e.rekey()
            ska.stream_sync()

        def as_copy():
            c = e.rekey(copy=True)
            ska.stream_sync()
            c.drop()

        def round_trip(keep=None):
            plain = ca.decrypt_packed(ska.download_packed(e.get()))
            s2 = skb.upload_compressed_string(cb.encrypt_compressed(plain, n - len(plain)))
            e2 = skb.store_put(s2)
            if keep is not None:
                keep.append(e2)
            else:
                e2.drop()

        kept = []
        round_trip(kept)                                             # warm-up: the second context's workspace; and the result
        assert cb.decrypt(kept[0].get()) == t
        kept[0].drop()
        s2 = skb.upload_compressed_string(cb.encrypt_compressed(t, 1))
        skb.stream_sync()

        def put():
            skb.store_put(s2).drop()

        t_trip = med(round_trip, a.reps)                             # before the in-place leg spoils the entry's contents
        t_put = med(put, a.reps)
        t_copy = med(as_copy, a.reps)
        t_in = med(in_place, a.reps)
        row = {"chars": n, "groups": (4 * n + 2047) // 2048, "entry_bytes": e.device_bytes,
               "rekey_in_place_ms_median": t_in[0], "rekey_in_place_ms_min": t_in[1],
               "rekey_copy_ms_median": t_copy[0], "rekey_copy_ms_min": t_copy[1],
               "round_trip_ms_median": t_trip[0], "round_trip_ms_min": t_trip[1],
               "put_ms_median": t_put[0], "put_ms_min": t_put[1],
               "rekey_in_place_over_put": t_in[0] / t_put[0], "round_trip_over_rekey_in_place": t_trip[0] / t_in[0]}
        res["rekey"].append(row)
        print(json.dumps(row), flush=True)
        e.drop()
        del s2
    last = res["rekey"][-1]
    res["criterion_rekey_4097_faster_than_put"] = bool(last["rekey_in_place_ms_median"] < last["put_ms_median"] and
                                                       last["rekey_copy_ms_median"] < last["put_ms_median"])
    for sk in (ska, skb):
        sk.close()
    for ck in (ca, cb):
        ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["criterion_rekey_4097_faster_than_put"]:
        sys.exit("re-key of the 4097-character entry is not faster than put: something is wrong")


if __name__ == "__main__":
    main()
