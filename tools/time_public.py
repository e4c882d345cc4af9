#!/usr/bin/env python3
"""Public-key (compact) strings on the MI355X: bytes handed over and upload time classic / seeded / public-key, the
extraction kernel beside the seeded expansion kernel, a config-5-shaped eq_ignore_case end to end with public-key
encryption, and the host cost and noise of the public encryption.

    python tools/time_public.py [--reps 5] [--out FILE.json] [--commit HASH]
    rocprofv3 --kernel-trace --stats ... -- python tools/time_public.py --kernels-only

Upload = host call + stream sync, the string already encrypted (classic: [n][4][2049] words through the pinned staging
buffer and one scatter launch; seeded: [n][4] bodies + destination pointers and one expansion launch; public-key: the
u32 masks of the groups touched, [n][4] u32 bodies + destination pointers and one extraction launch).  --kernels-only
uploads one 1024-character string (exactly 4096 blocks = one launch) both ways, alternating, and nothing else: under
`rocprofv3 --kernel-trace --stats` the averages of expand_public_blocks_kernel and expand_seeded_blocks_kernel are then
per 4096 blocks, written to the same pool blocks in the same run.  End to end: encryption + upload + eq_ignore_case
(fused, f64 FFT) + result download and decryption, two 4096-character strings + 1 padding (BASELINE config 5)."""
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
    ap.add_argument("--kernels-only", action="store_true", help="only the alternating 4096-block uploads (for a kernel trace)")
    a = ap.parse_args()
    ck = MyClientKey(0x7135)
    pp = ck.get_public_parameters()
    sk = MyServerKey.from_client_key(ck, arith=1)
    sk.set_mode(1)
    res = {"commit": a.commit, "reps": a.reps, "upload": [], "kernels_4096_blocks": {}, "eq_ignore_case_4096": {},
           "public_encrypt": {}}
    rng = np.random.default_rng(1)

    def synced(f):
        def g(x):
            s = f(x)
            sk.stream_sync()
            return s
        return g

    upload_classic = synced(sk.upload_string)
    upload_seeded = synced(sk.upload_compressed_string)
    upload_public = synced(sk.upload_compact_string)

    # one launch of each kernel on 4096 blocks, alternating: each string's blocks are released before the next upload, so
    # both kernels write the same pool blocks
    text = "".join(chr(v) for v in rng.integers(32, 127, 1023))
    cz, cp = ck.encrypt_compressed(text, 1), pp.encrypt(text, 1)
    tz, tp = [], []
    for _ in range(10 * a.reps):
        for f, c, ts in ((upload_seeded, cz, tz), (upload_public, cp, tp)):
            t0 = time.perf_counter()
            s = f(c)
            ts.append(time.perf_counter() - t0)
            del s
    res["kernels_4096_blocks"] = {"launches_each": 10 * a.reps, "seeded_upload_ms_median": statistics.median(tz) * 1e3,
                                  "public_upload_ms_median": statistics.median(tp) * 1e3}
    print("kernels", json.dumps(res["kernels_4096_blocks"]), flush=True)
    if a.kernels_only:
        sk.close()
        return

    for n in (64, 1024, 4097):
        text = "".join(chr(v) for v in rng.integers(32, 127, n - 1))
        cz, cp = ck.encrypt_compressed(text, 1), pp.encrypt(text, 1)
        x = cz.expand()
        assert np.array_equal(upload_public(cp).download(), cp.expand())
        upload_classic(x)                                            # warm the staging buffers and the pool
        tc, tz, tp = (med(lambda: f(v), a.reps) for f, v in ((upload_classic, x), (upload_seeded, cz), (upload_public, cp)))
        row = {"chars": n, "classic_bytes": int(x.nbytes), "seeded_bytes": int(cz.nbytes), "public_bytes": int(cp.nbytes),
               "classic_upload_ms_median": tc[0], "classic_upload_ms_min": tc[1],
               "seeded_upload_ms_median": tz[0], "seeded_upload_ms_min": tz[1],
               "public_upload_ms_median": tp[0], "public_upload_ms_min": tp[1]}
        res["upload"].append(row)
        print(json.dumps(row), flush=True)

    # host cost of the public encryption (4097 characters) and the noise of what it makes (one full group per call)
    text = "".join(chr(v) for v in rng.integers(32, 127, 4096))
    t = med(lambda: pp.encrypt(text, 1), a.reps)
    _, glwe = ck.secret_keys()
    errs = []
    for _ in range(8):
        full = pp.encrypt(text[:512], 0).expand().reshape(-1, 2049)
        dot = full[:, :2048][:, glwe.astype(bool)].sum(axis=1, dtype=np.uint64)
        msg = np.array([(ord(ch) >> (2 * b)) & 3 for ch in text[:512] for b in range(4)], np.uint64)
        errs.append((full[:, 2048] - dot - (msg << np.uint64(59))).view(np.int64).astype(np.float64))
    errs = np.concatenate(errs)
    s2 = float(glwe.sum())
    formula = np.sqrt((2.9403601535432533e-16 * 2.0 ** 64) ** 2 * (1024 + s2 + 1) + (2.0 ** 64 / 12) * (1 + s2))
    res["public_encrypt"] = {"chars": 4097, "ms_median": t[0], "ms_min": t[1], "groups_measured": 8,
                             "noise_rms_log2": float(np.log2(np.sqrt(np.mean(errs ** 2)))),
                             "noise_formula_log2": float(np.log2(formula)), "largest_error_log2": float(np.log2(np.abs(errs).max()))}
    print("public_encrypt", json.dumps(res["public_encrypt"]), flush=True)

    t1 = "".join(chr(v) for v in rng.integers(97, 123, 4096))
    t2 = t1.upper()

    def e2e_classic():
        r = sk.eq_ignore_case(ck.encrypt(t1, 1, None, sk), ck.encrypt(t2, 1, None, sk))
        assert ck.decrypt_char(r) == 1

    def e2e_seeded():
        s1 = sk.upload_compressed_string(ck.encrypt_compressed(t1, 1))
        s2 = sk.upload_compressed_string(ck.encrypt_compressed(t2, 1))
        assert ck.decrypt_char(sk.eq_ignore_case(s1, s2)) == 1

    def e2e_public():
        s1 = sk.upload_compact_string(pp.encrypt(t1, 1))
        s2 = sk.upload_compact_string(pp.encrypt(t2, 1))
        assert ck.decrypt_char(sk.eq_ignore_case(s1, s2)) == 1

    e2e_classic(); e2e_seeded(); e2e_public()                          # warm-up
    for name, f in (("classic", e2e_classic), ("seeded", e2e_seeded), ("public", e2e_public)):
        t = med(f, a.reps)
        res["eq_ignore_case_4096"][name] = {"ms_median": t[0], "ms_min": t[1]}
        print(name, json.dumps(res["eq_ignore_case_4096"][name]), flush=True)
    res["eq_ignore_case_4096"]["bytes_handed_over"] = {"classic": 2 * 4097 * 4 * 2049 * 8, "seeded": 2 * (48 + 32 * 4097),
                                                       "public": 2 * (16 + 8192 * 9 + 16 * 4097)}
    sk.close()
    ck.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
