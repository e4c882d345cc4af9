#!/usr/bin/env python3
"""Select by encrypted index on the MI355X: fhs_store_select on tables of 2 x 512, 256 x 64 and
64 x 64 characters parked as one entry each, and in the same process what the parent commit offers for the same row: the
re-key of the same entry (its nearest kernel: one keyswitch per group, one launch), a `get` of the row's window (the
route that tells the server which row is read), and find_clear + substr on 64 characters (the oblivious route there was:
one select per block per index bit, bootstraps).

    python tools/time_select.py [--reps 10] [--out FILE.json] [--commit HASH] [--machine NAME]
    rocprofv3 --kernel-trace --stats ... -- python tools/time_select.py --kernels-only

select = host call (one table pass of the raw query, the conversion launch, the CMux launches) + stream sync; the query
itself is made by the client beforehand and is not in the figure.  Where the tree has them (run on
an older tree the tool leaves these legs out, which is how the parent commit is timed in the same session): the seeded
form of every table, and fhs_store_select_batch on the 256 x 64 table at n = 1, 8, 32 and 64 seeded queries, ms per
call and per query and the bytes uploaded per query.  re-key = host call as a copy + stream sync; get = host call + stream
sync.  Medians after a warm-up round, all legs in one process.  No threshold is applied to any figure: the tool reports,
and the per-CMux time is given as a ratio to one re-key group of the same run (select time / launches against re-key
time: both are one workgroup deep per launch).
--kernels-only alternates a select and a re-key of the 256 x 64 table (32 groups: launches of 16, 8, 4, 2, 1 CMuxes and
three rotates, against one re-key launch of 32 groups) and nothing else: under `rocprofv3 --kernel-trace --stats` the
averages of select_cmux_kernel and rekey_glwe_kernel are then per launch in the same trace.
--batch-kernels N runs `reps` batch calls of N seeded queries on the 256 x 64 table and nothing else: under the same
profiler the call counts of select_query_to_ntt_kernel (1 per call) and select_cmux_kernel (8 per call) do not depend
on N, and their averages are per launch."""
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
from fhestring_amd.api import FheString, MyClientKey, MyServerKey, StoredString, select_bits  # noqa: E402

BATCHED = hasattr(StoredString, "select_many")                       # seeded queries and batches
BATCH_SIZES = (1, 8, 32, 64)

TABLES = ((2, 512), (256, 64), (64, 64))                             # rows x characters per row
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
    ap.add_argument("--kernels-only", action="store_true", help="only the alternating select / re-key of the 256 x 64 table")
    ap.add_argument("--batch-kernels", type=int, default=0, metavar="N", help="only batch calls of N seeded queries, 256 x 64")
    a = ap.parse_args()
    ck, other = MyClientKey(0x5E1EC7), MyClientKey(0x5E1EC8)
    sk = MyServerKey.from_client_key(ck, arith=1)
    sk.set_mode(1)
    sk.load_packing_key(ck)
    sk.load_rekey_key(ck.rekey_key(other))

    def table(rows, row_chars):
        """rows of row_chars - 1 characters and a NUL, uploaded, parked as ONE entry by put, the handles released"""
        texts = ["".join(chr(97 + (r + 3 * i) % 26) for i in range(row_chars - 1)) for r in range(rows)]
        chars = [ch for t in texts for ch in sk.upload_string(ck.encrypt_str_raw(t, 1)).chars]
        e = sk.store_put(FheString(chars))
        del chars
        return e, texts

    if a.batch_kernels:
        rows, row_chars = TABLES[1]
        e, texts = table(rows, row_chars)
        picks = [(7 * i + 3) % rows for i in range(a.batch_kernels)]
        qs = [ck.select_query(p, rows * row_chars, row_chars, seeded=True) for p in picks]
        for _ in range(a.reps):
            out = e.select_many(qs, row_chars)
            sk.stream_sync()
            for r in out[1:]:
                r.drop()
        assert ck.decrypt_packed(out[0].download_packed()) == texts[picks[0]]
        sk.close()
        ck.close()
        other.close()
        return

    if a.kernels_only:
        rows, row_chars = TABLES[1]
        e, texts = table(rows, row_chars)
        q = ck.select_query(rows - 3, rows * row_chars, row_chars)[0]
        for _ in range(10 * a.reps):
            r = e.select(q, row_chars)
            k = e.rekey(copy=True)
            sk.stream_sync()
            r.drop()
            k.drop()
        assert ck.decrypt_packed(e.select(q, row_chars).download_packed()) == texts[rows - 3]
        sk.close()
        ck.close()
        other.close()
        return

    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "tables": []}
    for rows, row_chars in TABLES:
        n = rows * row_chars
        e, texts = table(rows, row_chars)
        index = rows - 3 if rows > 2 else 1
        bits = select_bits(n, row_chars)
        q = ck.select_query(index, n, row_chars)[0]
        assert ck.decrypt_packed(e.select(q, row_chars).download_packed()) == texts[index]     # warm-up, and the result
        made = []

        def select():
            made.append(e.select(q, row_chars))
            sk.stream_sync()

        def rekey():
            made.append(e.rekey(copy=True))
            sk.stream_sync()

        def get():
            s = e.get(index * row_chars, row_chars)
            sk.stream_sync()
            del s

        rekey()
        get()
        ts, tr, tg = med(select, a.reps), med(rekey, a.reps), med(get, a.reps)
        tq = med(lambda: ck.select_query(index, n, row_chars), max(3, a.reps // 3))
        groups = (4 * n + 2047) // 2048
        row = {"rows": rows, "row_chars": row_chars, "groups": groups, "bits": bits, "launches": bits,
               "query_bytes": int(q.nbytes), "client_query_ms_median": tq[0],
               "select_ms_median": ts[0], "select_ms_min": ts[1],
               "rekey_copy_ms_median": tr[0], "rekey_copy_ms_min": tr[1],
               "get_row_ms_median": tg[0], "get_row_ms_min": tg[1],
               "select_per_launch_over_rekey": ts[0] / bits / tr[0], "select_over_get_row": ts[0] / tg[0]}
        if BATCHED:
            qs = ck.select_query(index, n, row_chars, seeded=True)
            assert ck.decrypt_packed(e.select(qs, row_chars).download_packed()) == texts[index]

            def select_seeded():
                made.append(e.select(qs, row_chars))
                sk.stream_sync()

            tss = med(select_seeded, a.reps)
            row.update({"seeded_query_bytes": int(qs.bodies.nbytes + qs.seed.nbytes),
                        "select_seeded_ms_median": tss[0], "select_seeded_ms_min": tss[1]})
        if BATCHED and (rows, row_chars) == TABLES[1]:
            row["batches"] = []
            for nq in BATCH_SIZES:
                picks = [(7 * i + 3) % rows for i in range(nq)]
                batch = [ck.select_query(p, n, row_chars, seeded=True) for p in picks]
                out = e.select_many(batch, row_chars)                                          # warm-up, and the results
                assert [ck.decrypt_packed(r.download_packed()) for r in out[:3]] == [texts[p] for p in picks[:3]]
                made.extend(out)

                def select_batch():
                    made.extend(e.select_many(batch, row_chars))
                    sk.stream_sync()

                tb = med(select_batch, a.reps)
                row["batches"].append({"n": nq, "form": "seeded", "ms_per_call_median": tb[0], "ms_per_call_min": tb[1],
                                       "ms_per_query_median": tb[0] / nq,
                                       "upload_bytes_per_query": int(batch[0].bodies.nbytes + batch[0].seed.nbytes) + 8})
                for x in made:
                    x.drop()
                del made[:]
        res["tables"].append(row)
        print(json.dumps(row), flush=True)
        for x in made + [e]:
            x.drop()

    # the oblivious route there was: the position found on the server, then substr at it, on 64 characters
    filler = "abcdefghijklmnopqrstuvwxy" * 3
    text = filler[:34] + PAT + filler[38:63]
    s = sk.upload_string(ck.encrypt_str_raw(text, 1))
    sk.stats(reset=True)
    r = sk.substr(s, sk.find_clear(s, PAT), 8)
    sk.flush()
    st = sk.stats()
    assert bytes(ck.decrypt_char_raw(b) for b in r.download()) == text[34:42].encode()
    del r

    def oblivious():
        r = sk.substr(s, sk.find_clear(s, PAT), 8)
        sk.flush()
        del r

    t = med(oblivious, a.reps)
    res["find_clear_substr_8_on_64"] = {"ms_median": t[0], "ms_min": t[1], "pbs_executed": st["pbs_executed"], "levels": st["levels"]}
    print(json.dumps(res["find_clear_substr_8_on_64"]), flush=True)
    sk.close()
    ck.close()
    other.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
