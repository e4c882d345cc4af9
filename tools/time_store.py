#!/usr/bin/env python3
"""Device-resident string store on the MI355X: put / get against the packed download for 64 / 1024 / 4097 characters, the
store's two kernels beside the seeded expansion kernel, and the point of the feature -- a contains_clear scan over a table
of 256 x 64-character strings read window by window from ONE parked entry against the same scan over the same strings
held as pool blocks.

    python tools/time_store.py [--reps 10] [--out FILE.json] [--commit HASH] [--machine NAME]
    rocprofv3 --kernel-trace --stats ... -- python tools/time_store.py --kernels-only

put = host call (it returns with the entry complete: the stream is synchronised inside), the string already on the
device; packed download = fhs_download_string_packed of the same handles in the same run (the same tree launches plus
the copy to the host); get = host call + stream sync.  Medians after a warm-up round, all legs in one process.
--kernels-only parks, restores and (seeded) uploads one 1024-character string (4096 blocks: one launch of each kernel),
alternating, and nothing else: under `rocprofv3 --kernel-trace --stats` the averages of store_switch32_kernel,
expand_public_blocks_kernel and expand_seeded_blocks_kernel are then per 4096 blocks in the same trace.
The scan: steps of 16 strings, one fhs_submit + fhs_pump per step (the flagship's level-skewed batching), fused DAG,
f64 FFT; the parked leg restores each string with get, records the operation and releases the handles, so at rest it
holds the entry alone."""
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

from fhestring_amd.api import FheString, MyClientKey, MyServerKey  # noqa: E402

POOL_BLOCK_BYTES = 16400                                             # 2050-word pool rows


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
    ap.add_argument("--kernels-only", action="store_true", help="only the alternating 4096-block put / get / seeded upload")
    a = ap.parse_args()
    ck = MyClientKey(0x7135)
    sk = MyServerKey.from_client_key(ck, arith=1)
    sk.set_mode(1)
    sk.load_packing_key(ck)
    rng = np.random.default_rng(1)
    text = lambda n: "".join(chr(v) for v in rng.integers(97, 123, n))

    def upload(t, padding=1):
        s = sk.upload_compressed_string(ck.encrypt_compressed(t, padding))
        sk.stream_sync()
        return s

    def get_synced(e, first=0, count=None):
        s = e.get(first, count)
        sk.stream_sync()
        return s

    if a.kernels_only:
        t = text(1023)
        cz = ck.encrypt_compressed(t, 1)
        s = upload(t)
        sk.store_put(s).drop()                                       # allocates the workspace
        for _ in range(10 * a.reps):
            e = sk.store_put(s)
            r = get_synced(e)
            z = sk.upload_compressed_string(cz)
            sk.stream_sync()
            del r, z
            e.drop()
        assert ck.decrypt(get_synced(sk.store_put(s))) == t
        sk.close()
        ck.close()
        return

    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "put_get": [], "scan_256x64": {}}
    for n in (64, 1024, 4097):
        t = text(n - 1)
        s = upload(t)
        e = sk.store_put(s)                                          # warm-up: workspace, staging buffers
        assert ck.decrypt(get_synced(e)) == ck.decrypt_packed(sk.download_packed(s)) == t
        entries = []

        def put():
            entries.append(sk.store_put(s))

        tp = med(put, a.reps)
        td = med(lambda: sk.download_packed(s), a.reps)
        tg = med(lambda: get_synced(e), a.reps)
        tw = med(lambda: get_synced(e, n // 2, min(64, n - n // 2)), a.reps)
        row = {"chars": n, "pool_bytes": 4 * n * POOL_BLOCK_BYTES, "entry_bytes": e.device_bytes,
               "put_ms_median": tp[0], "put_ms_min": tp[1],
               "packed_download_ms_median": td[0], "packed_download_ms_min": td[1],
               "put_over_packed_download": tp[0] / td[0],
               "get_ms_median": tg[0], "get_ms_min": tg[1],
               "get_window_64_ms_median": tw[0], "get_window_64_ms_min": tw[1]}
        res["put_get"].append(row)
        print(json.dumps(row), flush=True)
        for x in entries + [e]:
            x.drop()
        del s

    # the scan: 256 strings of 63 characters + 1 NUL, one entry of 16 384 characters
    n_str, n_chr, per_step = 256, 64, 16
    needle = "qzjx"
    texts = [text(n_chr - 1) for _ in range(n_str)]
    for i in range(0, n_str, 5):                                     # every fifth string holds the needle
        texts[i] = texts[i][:20] + needle + texts[i][24:]
    want = [int(needle in t) for t in texts]
    base_live = sk.stats()["blocks_live"]
    resident = [upload(t) for t in texts]
    resident_live = sk.stats()["blocks_live"] - base_live
    entry = sk.store_put(FheString([c for s in resident for c in s.chars]))
    sk.set_tick_balance()

    def scan(source):
        outs = []
        for step in range(n_str // per_step):
            for i in range(step * per_step, (step + 1) * per_step):
                s = source(i)
                outs.append(sk.contains_clear(s, needle))
                del s                                                # the recorded operation keeps what it needs
            sk.submit()
            sk.pump(1)
        sk.flush(wait=False)
        sk.stream_sync()
        return outs

    from_pool = lambda i: resident[i]
    from_store = lambda i: entry.get(i * n_chr, n_chr)
    for src in (from_pool, from_store):                              # warm-up, and the results
        assert [ck.decrypt_char(o) for o in scan(src)] == want
    t_pool, t_store = [], []
    for _ in range(a.reps):                                          # alternating: both legs see the same machine state
        for src, ts in ((from_pool, t_pool), (from_store, t_store)):
            t0 = time.perf_counter()
            outs = scan(src)
            ts.append(time.perf_counter() - t0)
            del outs
    m_pool, m_store = statistics.median(t_pool) * 1e3, statistics.median(t_store) * 1e3
    del resident
    parked_live = sk.stats()["blocks_live"] - base_live
    res["scan_256x64"] = {"strings": n_str, "chars_each": n_chr, "strings_per_step": per_step,
                          "resident_ms_median": m_pool, "resident_ms_min": min(t_pool) * 1e3,
                          "parked_ms_median": m_store, "parked_ms_min": min(t_store) * 1e3,
                          "parked_over_resident": m_store / m_pool,
                          "resident_ms_per_string": m_pool / n_str, "parked_ms_per_string": m_store / n_str,
                          "hbm_at_rest_resident_bytes": int(resident_live) * POOL_BLOCK_BYTES,
                          "hbm_at_rest_parked_bytes": sk.store_stats()["device_bytes"] + int(parked_live) * POOL_BLOCK_BYTES}
    print("scan", json.dumps(res["scan_256x64"]), flush=True)
    sk.close()
    ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
