#!/usr/bin/env python3
"""map_clear and class_flags on the MI355X next to to_upper, all legs in one process, f64-FFT arithmetic, fused mode.

    python tools/time_map.py [--reps 10] [--out profiles/r19_map.json] [--commit HASH] [--machine NAME]

On strings of 64 and 256 characters (text, one NUL of padding), in this order: `to_upper`, `map_clear` with the to_upper
table, `to_upper` again, `map_clear` with ROT13, `class_flags("A-Za-z0-9_")`.  The planner proves that the to_upper table
records to_upper's bootstraps and launch groups (tests/test_map.py), so the one judged figure is

    map_within_to_upper_N:  median(map_clear) <= min(median(to_upper), median(to_upper again)) + their difference

everything else is written down as measured.  One leg = record the operation + flush + stream sync on inputs that are
already resident; medians of --reps after one warm-up call, which also decrypts the result against Python once.
`expand_user_luts`: fhs_debug_read_lut on --tables fresh user tables (each call expands one table in front of the copy)
against the same calls once the tables are resident; the difference per table is the launch and the kernel."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

try:
    import torch  # noqa: F401  (one HIP runtime in the process: torch first, like bench.py)
except ImportError:
    pass

import numpy as np  # noqa: E402

import gen_map_plan as gen  # noqa: E402
from fhestring_amd.api import MyClientKey, MyServerKey  # noqa: E402

FILLER = "The quick brown fox_42 jumps over 7 lazy dogs; " * 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tables", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="")
    ap.add_argument("--machine", default="")
    a = ap.parse_args()
    ck = MyClientKey(0x71DE)
    sk = MyServerKey.from_client_key(ck, arith=1)
    sk.set_mode(1)
    res = {"commit": a.commit, "machine": a.machine, "reps": a.reps, "arith": "f64_fft", "legs": []}
    plain = lambda chars: bytes(ck.decrypt_char_raw(row) for row in chars.download())

    def leg(name, s, want, op):
        sk.flush()
        sk.stats(reset=True)
        got = plain(op(s))                                            # warm-up, and the result
        st, widths = sk.stats(), sk.level_widths()
        assert got == want, (name, len(s), got, want)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = op(s)
            sk.flush()
            del r
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        row = {"op": name, "chars": len(s), "ms_median": med, "ms_min": min(ts), "ms_max": max(ts),
               "spread": (max(ts) - min(ts)) / med, "pbs_executed": st["pbs_executed"], "pbs_extracted": st["pbs_extracted"],
               "levels": st["levels"], "level_widths": widths, "launch_groups": sk.launch_groups()[:len(widths)],
               "max_input_sum_c2": st["max_input_sum_c2"]}
        res["legs"].append(row)
        print(json.dumps(row), flush=True)
        return row

    member = sk.class_set(gen.CLASSES["identifier"])
    for n in (64, 256):
        text = FILLER[:n - 1]
        buf = text.encode() + bytes(1)
        s = sk.upload_string(ck.encrypt_str_raw(text, 1))
        up = gen.TABLES["to_upper"]
        first = leg("to_upper", s, buf.upper(), sk.to_upper)
        mapped = leg("map_clear(to_upper table)", s, buf.translate(up), lambda s: sk.map_clear(s, up))
        second = leg("to_upper again", s, buf.upper(), sk.to_upper)
        leg("map_clear(rot13)", s, buf.translate(gen.TABLES["rot13"]), lambda s: sk.map_clear(s, gen.TABLES["rot13"]))
        leg("class_flags('A-Za-z0-9_')", s, bytes(member[b >> 3] >> (b & 7) & 1 for b in buf),
            lambda s: sk.class_flags(s, gen.CLASSES["identifier"]))
        assert (mapped["pbs_executed"], mapped["level_widths"]) == (first["pbs_executed"], first["level_widths"])
        lo, hi = sorted((first["ms_median"], second["ms_median"]))
        res["map_over_to_upper_%d" % n] = mapped["ms_median"] / lo
        res["to_upper_difference_ms_%d" % n] = hi - lo
        res["map_within_to_upper_%d" % n] = bool(mapped["ms_median"] <= lo + (hi - lo))
        del s
    # the expansion kernel: fresh tables against resident ones through the same entry point
    L, h = sk.ctx._L, sk.ctx._h
    ids, out = [], np.zeros(2048, np.uint64)
    for k in range(a.tables):
        ids.append(sk.user_lut(bytes([(0x7A + k) & 31, (k >> 5) & 31, 29, 3] + [(k * 7 + j) & 31 for j in range(12)])))

    def read_all():
        t0 = time.perf_counter()
        for i in ids:
            sk.ctx._check(L.fhs_debug_read_lut(h, i, out.ctypes.data_as(C.c_void_p)))
        return (time.perf_counter() - t0) * 1e6 / len(ids)
    fresh = read_all()
    resident = min(read_all() for _ in range(3))
    res["expand_user_luts"] = {"tables": len(ids), "us_per_read_fresh": fresh, "us_per_read_resident": resident,
                               "us_per_table": fresh - resident}
    sk.close()
    ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}))


if __name__ == "__main__":
    main()
