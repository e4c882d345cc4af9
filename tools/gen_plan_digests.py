#!/usr/bin/env python3
"""Plan digests of the engine's host planner (tests/golden/plan_digests.json, checked by tests/test_plan_digest.py).

Every scenario records one operation on a fresh planner context (fhs_ctx_create_planner: the product's own DAG
construction, levelisation, rotation sharing and tick scheduling; nothing is computed, no GPU) and hashes what the engine
WOULD run.  A digest is SHA-256 over, in this order:

  1. the plan trace (fhs_debug_plan_trace / fhs_debug_plan_read), every block token replaced by the index of its first
     appearance -- the fixture pins the plan, not the planner's fake-pointer numbering;
  2. fhs_debug_char_terms of the result handles, under the same renaming;
  3. fhs_get_stats;  4. fhs_level_widths;  5. fhs_launch_groups;
  6. only where the trace names a user table (luts.h: ids from fhs_lut_catalogue_count() up are handed out process-wide in
     order of first registration): every such id in a row is replaced by the catalogue count plus the rank of its first
     appearance in the scenario, and the SHA-256 of each table's polynomial (fhs_debug_lut_poly), in that order, is hashed
     last -- the fixture pins which table a row applies, not what the process registered before.

The fhs_flush_plan / fhs_flush_level_exec / fhs_flush_level_commit walk writes no trace: its digest covers the per-level
(width, cap), the statistics after every exec, the level widths and the launch groups.

A digest that moves is a change of behaviour of the planner: the rows of a launch group, their order, the shared
extractions, the launch groups themselves or the statistics.  Regenerate (python tools/gen_plan_digests.py) only for a
change that is meant to do that.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_digests.json")
TR_UPLOAD, TR_ROW, TR_EXT, TR_GROUP_END = 1, 2, 3, 4
FHS_ERR_LIMIT = -4


def _read_words(sk, fn, *args):
    L, h = sk.ctx._L, sk.ctx._h
    n = C.c_size_t()
    sk.ctx._check(fn(h, *args, None, 0, C.byref(n)))
    buf = np.zeros(max(1, n.value), np.uint64)
    sk.ctx._check(fn(h, *args, buf.ctypes.data, n.value, C.byref(n)))
    return buf[:n.value]


def _trace_token_mask(t):
    """positions of the block tokens in a plan trace (include/fhestring_hip.h "plan trace")"""
    mask = np.zeros(len(t), bool)
    words = t.tolist()
    i = 0
    while i < len(words):
        tag = words[i]
        if tag == TR_UPLOAD:
            mask[i + 1] = True
            i += 2
        elif tag == TR_ROW:                           # out, lut, constant, n, (token, coefficient) x n
            n = words[i + 4]
            mask[i + 1] = True
            mask[i + 5:i + 5 + 2 * n:2] = True
            i += 5 + 2 * n
        elif tag == TR_EXT:                           # leader's out, own out, coefficient to extract
            mask[i + 1:i + 3] = True
            i += 4
        elif tag == TR_GROUP_END:
            i += 2
        else:
            raise ValueError("bad plan trace word %d at %d" % (tag, i))
    return mask


def _rename_user_tables(sk, t):
    """the `lut` word of every TR_ROW that names a user table -> catalogue count + rank of first appearance, in place;
    returns the content hashes of those tables in that order ([] when the trace names none)"""
    L = sk.ctx._L
    n_cat = L.fhs_lut_catalogue_count()
    words = t.tolist()
    rank, hashes = {}, []
    i = 0
    while i < len(words):
        tag = words[i]
        if tag == TR_ROW:
            lut = words[i + 2]
            if lut >= n_cat:
                if lut not in rank:
                    poly = np.zeros(2048, np.uint64)
                    assert L.fhs_debug_lut_poly(lut, poly.ctypes.data_as(C.c_void_p)) == 0
                    rank[lut] = len(rank)
                    hashes.append(hashlib.sha256(poly.tobytes()).hexdigest())
                t[i + 2] = n_cat + rank[lut]
            i += 5 + 2 * words[i + 4]
        else:
            i += {TR_UPLOAD: 2, TR_EXT: 4, TR_GROUP_END: 2}[tag]
    return hashes


def _terms_token_mask(t):
    """... in the fhs_debug_char_terms words of whole characters: [kind, value, n, (token, coefficient) x n] per block"""
    mask = np.zeros(len(t), bool)
    words = t.tolist()
    i = 0
    while i < len(words):
        n = words[i + 2]
        mask[i + 3:i + 3 + 2 * n:2] = True
        i += 3 + 2 * n
    return mask


def _rename(parts):
    """[(words, token mask)] -> the words of all parts, tokens numbered by first appearance across the parts"""
    words = np.concatenate([w for w, _ in parts]) if parts else np.zeros(0, np.uint64)
    mask = np.concatenate([m for _, m in parts]) if parts else np.zeros(0, bool)
    tok = words[mask]
    if len(tok):
        _, first, inv = np.unique(tok, return_index=True, return_inverse=True)
        rank = np.empty(len(first), np.uint64)
        rank[np.argsort(first, kind="stable")] = np.arange(len(first), dtype=np.uint64)
        words = words.copy()
        words[mask] = rank[inv.reshape(-1)]
    return words


def _hash(*chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c if isinstance(c, bytes) else json.dumps(c, sort_keys=True).encode())
        h.update(b"|")
    return h.hexdigest()


def _chars_of(result):
    from fhestring_amd.api import FheAsciiChar, FheSplit, FheU16
    if isinstance(result, FheAsciiChar):
        return [result]
    if hasattr(result, "chars"):
        return list(result.chars)
    if isinstance(result, FheU16):
        return [result.lo, result.hi]
    if isinstance(result, FheSplit):
        return _chars_of(result.buffers) + [result.pattern_found]
    out = []
    for r in result:
        out.extend(_chars_of(r))
    return out


def record(body, mode=1, setup=None):
    """one scenario on a fresh planner context -> its digest.  A body that ends in an error of the library (FhsError, or
    the OverflowError the binding makes of FHS_ERR_LIMIT) digests the error code with the statistics and the plan trace
    recorded up to that point; a digest without an error is what it was before errors were digested."""
    from fhestring_amd import FhsError
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        L, h = sk.ctx._L, sk.ctx._h
        sk.set_mode(mode)
        if setup:
            setup(sk)
        sk.ctx._check(L.fhs_debug_plan_trace(h, 1))
        sk.stats(reset=True)
        result, error = [], []
        try:
            result = body(sk)
        except FhsError as err:
            error = [{"error": err.code}]
        except OverflowError:
            error = [{"error": FHS_ERR_LIMIT}]
        trace = _read_words(sk, L.fhs_debug_plan_read)            # flushes
        tables = _rename_user_tables(sk, trace)
        parts = [(trace, _trace_token_mask(trace))]
        for ch in _chars_of(result):
            t = _read_words(sk, L.fhs_debug_char_terms, C.c_uint64(ch.h))
            parts.append((t, _terms_token_mask(t)))
        return _hash(_rename(parts).tobytes(), sk.stats(), sk.level_widths(), sk.launch_groups(), *error,
                     *([{"user_tables": tables}] if tables else []))
    finally:
        sk.close()


def level_walk(rank, world=2):
    """fhs_dist_config + fhs_flush_plan / fhs_flush_level_exec / fhs_flush_level_commit over replace 257 / 3 / 2"""
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        L, h = sk.ctx._L, sk.ctx._h
        sk.set_mode(1)
        sk.set_auto_flush(0)
        sk.ctx._check(L.fhs_dist_config(h, rank, world))
        s, f, t = sk.dummy_string(257), sk.dummy_string(3), sk.dummy_string(2)
        out = sk.replace(s, f, t)
        sk.stats(reset=True)
        n_levels, max_w = C.c_uint64(), C.c_uint64()
        sk.ctx._check(L.fhs_flush_plan(h, C.byref(n_levels), C.byref(max_w)))
        dummy = (C.c_uint64 * 1)()
        walk = [[n_levels.value, max_w.value]]
        for k in range(n_levels.value):
            width, cap = C.c_uint64(), C.c_uint64()
            sk.ctx._check(L.fhs_flush_level_exec(h, k, dummy, C.byref(width), C.byref(cap)))
            walk.append([width.value, cap.value, sk.stats()])
            sk.ctx._check(L.fhs_flush_level_commit(h, k, dummy))
        del out
        return _hash(walk, sk.stats(), sk.level_widths(), sk.launch_groups())
    finally:
        sk.close()


def _contains(pattern, sharing, balance):
    def setup(sk):
        sk.ctx.set_rotation_sharing(sharing)
        sk.set_tick_balance(balance)
    return lambda: record(lambda sk: sk.contains_clear(sk.dummy_string(65), pattern), setup=setup)


def _replace(auto_flush, balance):
    def setup(sk):
        sk.set_auto_flush(auto_flush)
        sk.set_tick_balance(balance)
    return lambda: record(lambda sk: sk.replace(sk.dummy_string(1025), sk.dummy_string(5), sk.dummy_string(5)), setup=setup)


def _requests(balance):
    def body(sk):
        keep = []
        for s in [sk.dummy_string(65) for _ in range(4)]:
            keep.append(sk.contains_clear(s, "a2S$"))
            sk.submit()
            sk.pump(1)
        sk.flush()
        return keep
    return lambda: record(body, setup=lambda sk: sk.set_tick_balance(balance))


def _compressed(sk):
    from fhestring_amd.api import FheString, FheAsciiChar
    n = 70                                              # any bytes of the right size: a planner reads none of them
    seed, bodies = np.zeros(8, np.uint32), np.zeros(4 * n, np.uint64)
    hs = (C.c_uint64 * n)()
    sk.ctx._check(sk.ctx._L.fhs_upload_string_compressed(sk.ctx._h, seed.ctypes.data, bodies.ctypes.data, n, 3, hs))
    return sk.contains_clear(FheString([FheAsciiChar(sk, hs[i]) for i in range(n)]), "abcd")


def _public(sk):
    from fhestring_amd.api import FheString, FheAsciiChar
    n_total, first, n = 600, 20, 70
    mask32, body32 = np.zeros(2 * 2048, np.uint32), np.zeros(4 * n_total, np.uint32)
    hs = (C.c_uint64 * n)()
    sk.ctx._check(sk.ctx._L.fhs_upload_string_public(sk.ctx._h, mask32.ctypes.data, body32.ctypes.data, n_total, first, n, hs))
    return sk.contains_clear(FheString([FheAsciiChar(sk, hs[i]) for i in range(n)]), "abcd")


def _pair_4097(op):
    return lambda: record(lambda sk: getattr(sk, op)(sk.dummy_string(4097), sk.dummy_string(4097)))


SCENARIOS = {}
for _pat, _name in (("abcd", "abcd"), ("a2S$", "a2S")):
    for _sh in (True, False):
        for _bal in (0, 1024):
            SCENARIOS["contains_clear_65_%s_%s_%s" % (_name, "shared" if _sh else "unshared",
                                                      "balance%d" % _bal if _bal else "nobalance")] = _contains(_pat, _sh, _bal)
SCENARIOS.update({
    "find_clear_257_balance1024": lambda: record(lambda sk: sk.find_clear(sk.dummy_string(257), "a2S$"),
                                                 setup=lambda sk: sk.set_tick_balance(1024)),
    "find_257_enc4": lambda: record(lambda sk: sk.find(sk.dummy_string(257), sk.dummy_string(4))),
    "le_4097": _pair_4097("le"),
    "eq_ignore_case_4097": _pair_4097("eq_ignore_case"),
    "replace_1025_5_5_auto8192_balance1024": _replace(8192, 1024),
    "replace_1025_5_5_auto0": _replace(0, 0),
    "replace_1025_5_5_auto8192_nobalance": _replace(8192, 0),
    "four_requests_submit_pump_balance1024": _requests(1024),
    "four_requests_submit_pump_nobalance": _requests(0),
    # (levels of 496 / 130 rows never reach a 1 024-slot round: a round of 64 makes the alignment split them)
    "contains_clear_65_a2S_shared_balance64": _contains("a2S$", True, 64),
    "four_requests_submit_pump_balance64": _requests(64),
    "as_written_contains_clear_65": lambda: record(lambda sk: sk.contains_clear(sk.dummy_string(65), "abcd"), mode=0),
    "upload_compressed_contains_clear_70": lambda: record(_compressed),
    "upload_public_contains_clear_70": lambda: record(_public),
    "level_walk_replace_257_3_2_rank0of2": lambda: level_walk(0),
    "level_walk_replace_257_3_2_rank1of2": lambda: level_walk(1),
})


def main():
    out = {name: fn() for name, fn in SCENARIOS.items()}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d digests to %s" % (len(out), os.path.relpath(FIXTURE, ROOT)))


if __name__ == "__main__":
    main()
