#!/usr/bin/env python3
"""Packed result download on the MI355X: classic `download + decrypt` against `download_packed + decrypt_packed` for
64 / 1024 / 4097 characters, and to_upper on 4097 characters end to end with either download.

    python tools/time_packed.py [--reps 10] [--out FILE.json] [--commit HASH] [--machine NAME]

Download = host call that returns with the data on the host (the context's stream is synchronised inside), the string
already on the device; decrypt = the client's host code.  Medians after one warm-up round, one process, one run.  The
per-level kernel times: `rocprofv3 --kernel-trace --stats -- python tools/time_packed.py --trace-only` (one
4097-character packed download after warm-up of the workspace).  End to end: client encryption, compressed upload,
to_upper (fused, f64 FFT), download, decryption."""
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
    ap.add_argument("--trace-only", action="store_true", help="one 4097-character packed download, for a kernel trace")
    a = ap.parse_args()
    ck = MyClientKey(0x7135)
    sk = MyServerKey.from_client_key(ck, arith=1)
    sk.set_mode(1)
    sk.load_packing_key(ck)
    rng = np.random.default_rng(1)
    text = lambda n: "".join(chr(v) for v in rng.integers(97, 123, n))

    if a.trace_only:
        t = text(4096)
        s = sk.upload_compressed_string(ck.encrypt_compressed(t, 1))
        sk.download_packed(s)                                        # allocates the workspace
        sk.stream_sync()
        assert ck.decrypt_packed(sk.download_packed(s)) == t
        sk.close()
        ck.close()
        return

    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "download": [], "to_upper_4097": {}}
    for n in (64, 1024, 4097):
        t = text(n - 1)
        s = sk.upload_compressed_string(ck.encrypt_compressed(t, 1))
        sk.stream_sync()
        classic = lambda: ck.decrypt_str_raw(s.download())
        packed = lambda: ck.decrypt_packed(sk.download_packed(s))
        assert classic() == packed() == t                            # warm-up: staging buffers, workspace
        row = {"chars": n, "classic_bytes": n * 4 * 2049 * 8, "packed_bytes": sk.download_packed(s).nbytes}
        for name, dl, dec in (("classic", s.download, ck.decrypt_str_raw), ("packed", lambda: sk.download_packed(s), ck.decrypt_packed)):
            x = dl()
            td, tc, tt = med(dl, a.reps), med(lambda: dec(x), a.reps), med(lambda: dec(dl()), a.reps)
            row[name] = {"download_ms_median": td[0], "download_ms_min": td[1], "decrypt_ms_median": tc[0],
                         "total_ms_median": tt[0], "total_ms_min": tt[1]}
        row["speedup_total"] = row["classic"]["total_ms_median"] / row["packed"]["total_ms_median"]
        res["download"].append(row)
        print(json.dumps(row), flush=True)

    t = text(4096)

    def e2e(packed):
        up = sk.to_upper(sk.upload_compressed_string(ck.encrypt_compressed(t, 1)))
        got = ck.decrypt_packed(sk.download_packed(up)) if packed else ck.decrypt(up)
        assert got == t.upper()

    e2e(False); e2e(True)                                            # warm-up
    for name, flag in (("classic", False), ("packed", True)):
        m = med(lambda: e2e(flag), a.reps)
        res["to_upper_4097"][name] = {"ms_median": m[0], "ms_min": m[1]}
        print("to_upper_4097", name, json.dumps(res["to_upper_4097"][name]), flush=True)
    sk.close()
    ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
