#!/usr/bin/env python3
"""Compressed (seeded) strings on the MI355X: bytes handed over and upload time classic vs compressed, the device
expansion alone, and a config-5-shaped eq_ignore_case end to end both ways.

    python tools/time_compressed.py [--reps 5] [--out FILE.json] [--commit HASH]

Upload = host call + stream sync, the string already encrypted (classic: [n][4][2049] words through the pinned staging
buffer and one scatter launch; compressed: [n][4] bodies + destination pointers and one expansion launch).  The
expansion alone: the kernel times of expand_seeded_blocks_kernel in a run under `rocprofv3 --kernel-trace --stats -- python
tools/time_compressed.py` (4096 blocks per launch).  End to end: client encryption +
upload + eq_ignore_case (fused, f64 FFT) + result download and decryption, two 4096-character strings + 1 padding
(BASELINE config 5)."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="")
    a = ap.parse_args()
    ck = MyClientKey(0x7135)
    sk = MyServerKey.from_client_key(ck, arith=1)
    sk.set_mode(1)
    res = {"commit": a.commit, "reps": a.reps, "upload": [], "expansion": {}, "eq_ignore_case_4096": {}}
    rng = np.random.default_rng(1)

    def upload_classic(x):
        s = sk.upload_string(x)
        sk.stream_sync()
        return s

    def upload_compressed(c):
        s = sk.upload_compressed_string(c)
        sk.stream_sync()
        return s

    for n in (64, 1024, 4097):
        text = "".join(chr(v) for v in rng.integers(32, 127, n - 1))
        c = ck.encrypt_compressed(text, 1)
        x = c.expand()
        assert np.array_equal(upload_compressed(c).download(), x)
        upload_classic(x)                                            # warm the staging buffers and the pool
        tc = med(lambda: upload_classic(x), a.reps)
        tz = med(lambda: upload_compressed(c), a.reps)
        row = {"chars": n, "classic_bytes": int(x.nbytes), "compressed_bytes": int(c.nbytes),
               "ratio": x.nbytes / c.nbytes, "classic_upload_ms_median": tc[0], "classic_upload_ms_min": tc[1],
               "compressed_upload_ms_median": tz[0], "compressed_upload_ms_min": tz[1]}
        res["upload"].append(row)
        print(json.dumps(row), flush=True)

    c = ck.encrypt_compressed("".join(chr(v) for v in rng.integers(32, 127, 4096)), 1)
    t = med(lambda: upload_compressed(c), 2 * a.reps)
    res["expansion"] = {"chars": len(c), "blocks": 4 * len(c), "upload_ms_median": t[0], "upload_ms_min": t[1]}
    print("expansion", json.dumps(res["expansion"]), flush=True)

    t1 = "".join(chr(v) for v in rng.integers(97, 123, 4096))
    t2 = t1.upper()

    def e2e_classic():
        r = sk.eq_ignore_case(ck.encrypt(t1, 1, None, sk), ck.encrypt(t2, 1, None, sk))
        assert ck.decrypt_char(r) == 1

    def e2e_compressed():
        s1 = sk.upload_compressed_string(ck.encrypt_compressed(t1, 1))
        s2 = sk.upload_compressed_string(ck.encrypt_compressed(t2, 1))
        assert ck.decrypt_char(sk.eq_ignore_case(s1, s2)) == 1

    e2e_classic(); e2e_compressed()                                   # warm-up
    for name, f in (("classic", e2e_classic), ("compressed", e2e_compressed)):
        t = med(f, a.reps)
        res["eq_ignore_case_4096"][name] = {"ms_median": t[0], "ms_min": t[1]}
        print(name, json.dumps(res["eq_ignore_case_4096"][name]), flush=True)
    res["eq_ignore_case_4096"]["bytes_handed_over"] = {"classic": 2 * 4097 * 4 * 2049 * 8, "compressed": 2 * (48 + 32 * 4097)}
    sk.close()
    ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
