#!/usr/bin/env python3
"""Wall time of the host-only helper code (client key generation, string encryption, host expansions, host packing) and
of the two key loads that end in device work, for an A/B of two builds of the library
(profiles/r14_host_helpers_ab.json; docs/HISTORY.md section 17).

    python tools/time_host_helpers.py --cpu                      one JSON line: this build's CPU figures (seconds)
    python tools/time_host_helpers.py --gpu                      one JSON line: load_server_key / load_multibit_key
                                                                 under the exact arithmetic on GPU 0, host clock
    python tools/time_host_helpers.py --ab PARENT.so --cpu|--gpu [--runs N] --out FILE
        alternates the parent build (FHS_LIB_PATH=PARENT.so) and this tree's build in fresh processes confined to 16 CPUs
        with taskset, one discarded round first, and merges runs, medians, spreads and the acceptance bound
        (new median <= parent median + parent spread, spread = max - min) into FILE.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0xF5E57121
CPUS = "0-15"


def _timed(out, name, f):
    t0 = time.perf_counter()
    r = f()
    out[name + "_s"] = round(time.perf_counter() - t0, 4)
    return r


def cpu_figures():
    import numpy as np
    import fhestring_amd
    from fhestring_amd import api
    fhestring_amd.lib()                                      # loading the library (and torch before it) is not timed
    out = {}
    ck = _timed(out, "seeded_client_create", lambda: api.MyClientKey(SEED))
    _timed(out, "first_bsk_mb2", ck.bsk_mb2)
    csk = _timed(out, "first_compressed_server_key", ck.compressed_server_key)
    _timed(out, "expand_compressed_server_key", lambda: api.expand_compressed_server_key(*csk))
    key = _timed(out, "first_packing_key", ck.packing_key)
    text = "a" * 4097
    buf = np.empty((4097, 4, 2049), np.uint64)
    buf[:] = 0                                               # page the buffer in outside the timed region
    assert _timed(out, "encrypt_decrypt_str_4097", lambda: ck.decrypt_str_raw(ck.encrypt_str_raw(text, 0, out=buf))) == text
    pp = ck.get_public_parameters()
    pp.set_insecure_seed(1)
    _timed(out, "public_encrypt_4097", lambda: pp.encrypt(text, 0))
    _timed(out, "pack_host_2048_blocks", lambda: api.pack_host(key, buf.reshape(-1, 2049)[:2048]))
    return out


def gpu_figures():
    import fhestring_amd
    from fhestring_amd import api
    ck = api.MyClientKey(SEED)
    bsk, ksk, mb2 = ck.bsk(), ck.ksk(), ck.bsk_mb2()
    ctx = fhestring_amd.Context(0)
    ctx.set_arithmetic(ctx.ARITH_EXACT_NTT)
    out = {}
    _timed(out, "load_server_key_exact", lambda: ctx.load_server_key(bsk, ksk))       # the call returns synchronised
    _timed(out, "load_multibit_key_exact", lambda: ctx.load_multibit_key(mb2))
    ctx.close()
    return out


def ab(parent, mode, runs, path):
    cmd = ["taskset", "-c", CPUS, sys.executable, os.path.abspath(__file__), mode]
    sides = {"parent": dict(os.environ, FHS_LIB_PATH=os.path.abspath(parent)),
             "new": {k: v for k, v in os.environ.items() if k != "FHS_LIB_PATH"}}
    got = {"parent": [], "new": []}
    for r in range(runs + 1):                                # round 0 is discarded
        for side, env in sides.items():
            line = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=120).stdout
            if r:
                got[side].append(json.loads(line.strip().splitlines()[-1]))
    rec = {}
    for name in got["new"][0]:
        cell = {}
        for side in ("parent", "new"):
            v = [g[name] for g in got[side]]
            cell[side] = {"runs": v, "median": statistics.median(v), "min": min(v), "max": max(v),
                          "spread": round(max(v) - min(v), 4)}
        cell["criterion"] = "new median <= parent median + parent spread"
        cell["bound"] = round(cell["parent"]["median"] + cell["parent"]["spread"], 4)
        cell["met"] = cell["new"]["median"] <= cell["bound"]
        rec[name] = cell
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["%s_%d_runs_each_on_cpus_%s" % (mode.strip("-"), runs, CPUS)] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({n: (c["parent"]["median"], c["new"]["median"], c["met"]) for n, c in rec.items()}))
    return all(c["met"] for c in rec.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--ab", metavar="PARENT.so")
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.cpu != a.gpu, "one of --cpu / --gpu"
    if a.ab:
        ab(a.ab, "--cpu" if a.cpu else "--gpu", a.runs or (7 if a.cpu else 3), a.out)
    else:
        print(json.dumps(cpu_figures() if a.cpu else gpu_figures()))


if __name__ == "__main__":
    main()
