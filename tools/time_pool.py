#!/usr/bin/env python3
"""Block pool trimming on the MI355X: what a context holds after a string was ingested, parked and
its handles released, what a trim gives back and how long it takes -- and, from a kernel trace, the time of the
compaction's move kernel beside the download's gather kernel.

    python tools/time_pool.py [--out FILE.json] [--commit HASH] [--machine NAME]
        64 / 1024 / 4097 characters, each in a FRESH context (fhs_debug_live_resources()[0] is process-wide: a pool kept
        from an earlier size would count in the next row): upload, store_put, release of the handles, compacting trim.
        A fourth row keeps every other character of 4097 instead of parking them, so that the trim has blocks to move.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_pool.py --kernel-workload COUNTS.json
        in a run of its own: 4096 characters of random words, every other one released; the 8192 surviving blocks are
        downloaded (gather_rows_kernel, scattered sources), 4096 of them are moved by the trim (pool_move_blocks_kernel)
        and all are downloaded again and compared.  COUNTS.json receives the rows each kernel handled.
    python tools/time_pool.py --kernel-stats DIR --counts COUNTS.json --out FILE.json
        no GPU: reads the trace's kernel_stats.csv and adds both kernels' time per 4096 rows to FILE.json.
Both kernels move the same bytes through a pointer table; the criterion, written down and not tuned, is
    move time per 4096 blocks <= 1.25 x gather time per 4096 rows, in the same trace
(the margin covers scattered instead of dense writes); the exit status of the last form says whether it held."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK_BYTES = 2048 * 2050 * 8
MARGIN = 1.25


def device_imports():
    try:
        import torch  # noqa: F401  (one HIP runtime in the process: torch first, like bench.py)
    except ImportError:
        pass
    import numpy as np
    from fhestring_amd._lib import live_resources
    from fhestring_amd.api import FheString, MyClientKey, MyServerKey
    return np, live_resources, FheString, MyClientKey, MyServerKey


def trim_rows(a):
    np, live_resources, FheString, MyClientKey, MyServerKey = device_imports()
    rng = np.random.default_rng(1)
    ck = MyClientKey(0x7135)
    rows = []
    for n, keep_every in ((64, 0), (1024, 0), (4097, 0), (4097, 2)):
        sk = MyServerKey.from_client_key(ck, arith=1)                # a fresh context per row
        sk.set_mode(1)
        sk.load_packing_key(ck)
        base = live_resources()[0]                                   # keys, tables: what the context holds without a pool
        text = "".join(chr(v) for v in rng.integers(97, 123, n - 1))
        s = sk.upload_compressed_string(ck.encrypt_compressed(text, 1))
        peak_blocks = sk.pool_stats()["live"]
        if keep_every:
            kept = FheString([s.chars[i] for i in range(0, n, keep_every)])
            e = None
        else:
            kept = None
            e = sk.store_put(s)
        del s
        before, st0 = live_resources()[0], sk.pool_stats()
        t0 = time.perf_counter()
        r = sk.pool_trim(compact=True)
        ms = (time.perf_counter() - t0) * 1e3
        after, st1 = live_resources()[0], sk.pool_stats()
        assert before - after == r["bytes_released"] == st0["device_bytes"] - st1["device_bytes"]
        if e is not None:
            assert ck.decrypt(e.get()).rstrip("\0") == text
        else:
            assert ck.decrypt(kept).rstrip("\0") == text[::keep_every]
        row = {"chars": n, "leg": "parked, handles released" if e is not None else "every %d. character kept" % keep_every,
               "peak_live_blocks": peak_blocks, "live_blocks_at_trim": st0["live"],
               "chunks_before": st0["chunks"], "chunks_after": st1["chunks"],
               "store_bytes": sk.store_stats()["device_bytes"],
               "pool_bytes_before": st0["device_bytes"], "pool_bytes_after": st1["device_bytes"],
               "live_device_bytes_before": before, "live_device_bytes_after": after,
               "live_device_bytes_without_pool": base,
               "blocks_moved": r["blocks_moved"], "bytes_released": r["bytes_released"], "trim_wall_ms": ms}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del kept, e
        sk.close()
    ck.close()
    return rows


def kernel_workload(counts_path):
    np, live_resources, FheString, MyClientKey, MyServerKey = device_imports()
    ck = MyClientKey(0x7135)
    sk = MyServerKey.from_client_key(ck, arith=1)
    rng = np.random.default_rng(2)
    n = 4096
    rows = rng.integers(0, 1 << 64, (n, 4, 2049), dtype=np.uint64)
    s = sk.upload_string(rows)
    kept = FheString(s.chars[0::2])
    del s
    want = rows[0::2]
    del rows
    assert np.array_equal(kept.download(), want)                     # 8192 rows gathered from eight half-full chunks
    r = sk.pool_trim(compact=True)
    assert r == {"blocks_moved": 4096, "bytes_released": 4 * CHUNK_BYTES}, r
    assert np.array_equal(kept.download(), want)                     # ... and from the four chunks that are left
    with open(counts_path, "w") as f:
        json.dump({"gather_rows_kernel": 2 * 4 * len(kept), "pool_move_blocks_kernel": r["blocks_moved"]}, f)
    del kept
    sk.close()
    ck.close()


def kernel_stats(trace_dir, counts_path):
    with open(counts_path) as f:
        counts = json.load(f)
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for rec in csv.DictReader(f):
                for name, n_rows in counts.items():
                    if name in rec["Name"]:
                        k = out.setdefault(name, {"calls": 0, "total_ns": 0, "rows": n_rows})
                        k["calls"] += int(rec["Calls"])
                        k["total_ns"] += int(rec["TotalDurationNs"])
    for k in out.values():
        k["us_per_4096_rows"] = k["total_ns"] / 1e3 / k["rows"] * 4096
        k["GB_per_s_read_plus_written"] = 2 * k["rows"] * 2049 * 8 / k["total_ns"]
    if set(out) != set(counts):
        sys.exit("kernel_stats.csv under %s lacks a kernel of %s" % (trace_dir, sorted(counts)))
    ratio = out["pool_move_blocks_kernel"]["us_per_4096_rows"] / out["gather_rows_kernel"]["us_per_4096_rows"]
    return {"kernels": out, "move_over_gather": ratio, "margin": MARGIN, "criterion_move_within_margin": bool(ratio <= MARGIN)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="")
    ap.add_argument("--machine", default="")
    ap.add_argument("--kernel-workload", default=None, metavar="COUNTS.json")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    ap.add_argument("--counts", default=None)
    a = ap.parse_args()
    if a.kernel_workload:
        return kernel_workload(a.kernel_workload)
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.kernel_stats:
        res["kernel_trace"] = kernel_stats(a.kernel_stats, a.counts)
    else:
        res.update({"commit": a.commit, "machine": a.machine, "pool_trim": trim_rows(a)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    if a.kernel_stats and not res["kernel_trace"]["criterion_move_within_margin"]:
        sys.exit("the move kernel took more than %.2f x the gather kernel's time per 4096 rows" % MARGIN)


if __name__ == "__main__":
    main()
