"""Block pool accounting and trimming on the host (include/fhestring_hip.h, "block pool"): the three
entry points and their prototypes, argument and state errors, a planner context (which holds no chunk), and the victim
choice of a compacting trim, fhs_debug_pool_plan, on chosen occupancies.  The move itself runs on the device:
_smoke_pool_trim of __graft_entry__.py (tests/test_pool_trim_device.py runs that step alone)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FHS_ERR_ARG, FHS_ERR_STATE = -1, -3
CHUNK = 2048


@pytest.fixture(scope="module")
def L():
    from fhestring_amd import lib
    return lib()


def _plan(L, live, keep):
    live = np.array(live, np.uint32)
    victim = np.full(max(1, live.size), 7, np.uint8)
    assert L.fhs_debug_pool_plan(live.ctypes.data_as(C.c_void_p), live.size, keep, victim.ctypes.data_as(C.c_void_p)) == 0
    return victim[:live.size].tolist()


def test_entry_points_have_the_headers_prototypes(L):
    from fhestring_amd import cabi
    funcs = {name: (ret, args) for name, ret, args in cabi.parse_header()["funcs"]}
    T = cabi.CType
    assert funcs["fhs_pool_stats"] == (T("int", False, 0), [("ctx", T("fhs_ctx", False, 1)), ("out", T("uint64_t", False, 1))])
    assert funcs["fhs_pool_trim"] == (T("int", False, 0), [
        ("ctx", T("fhs_ctx", False, 1)), ("mode", T("int", False, 0)), ("keep_free_blocks", T("size_t", False, 0)),
        ("blocks_moved", T("uint64_t", False, 1)), ("bytes_released", T("uint64_t", False, 1))])
    assert funcs["fhs_debug_pool_plan"] == (T("int", False, 0), [
        ("live_per_chunk", T("uint32_t", True, 1)), ("n_chunks", T("size_t", False, 0)),
        ("keep_free_blocks", T("size_t", False, 0)), ("victim_out", T("uint8_t", False, 1))])
    consts = dict(cabi.parse_header()["consts"])
    assert (consts["FHS_TRIM_RELEASE"], consts["FHS_TRIM_COMPACT"]) == (0, 1)
    for name in ("fhs_pool_stats", "fhs_pool_trim", "fhs_debug_pool_plan"):       # ... and the library exports them
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == len(funcs[name][1]), name
    assert L.fhs_pool_trim.argtypes[1:3] == [C.c_int, C.c_size_t]


def test_argument_errors(L):
    from fhestring_amd.api import MyServerKey
    out, moved = (C.c_uint64 * 6)(), C.c_uint64(5)
    assert L.fhs_pool_stats(None, out) == FHS_ERR_ARG
    assert L.fhs_pool_trim(None, 0, 0, None, None) == FHS_ERR_ARG
    sk = MyServerKey.planner()
    try:
        h = sk.ctx._h
        assert L.fhs_pool_stats(h, None) == FHS_ERR_ARG
        for mode in (-1, 2, 77):
            assert L.fhs_pool_trim(h, mode, 0, C.byref(moved), None) == FHS_ERR_ARG, mode
        assert L.fhs_pool_trim(h, 0, 0, None, None) == 0 and L.fhs_pool_trim(h, 1, 5, None, None) == 0   # outputs may be NULL
    finally:
        sk.close()
    one, v = np.array([3], np.uint32), np.zeros(1, np.uint8)
    assert L.fhs_debug_pool_plan(None, 1, 0, v.ctypes.data_as(C.c_void_p)) == FHS_ERR_ARG
    assert L.fhs_debug_pool_plan(one.ctypes.data_as(C.c_void_p), 1, 0, None) == FHS_ERR_ARG
    assert L.fhs_debug_pool_plan(None, 0, 0, None) == 0                           # no chunk: nothing to write
    over = np.array([CHUNK + 1], np.uint32)                                       # more live blocks than a chunk holds
    assert L.fhs_debug_pool_plan(over.ctypes.data_as(C.c_void_p), 1, 0, v.ctypes.data_as(C.c_void_p)) == FHS_ERR_ARG


def test_planner_context_reports_live_and_trims_nothing():
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        zero = {"chunks": 0, "blocks_per_chunk": CHUNK, "live": 0, "free": 0, "free_pending": 0, "device_bytes": 0}
        assert sk.pool_stats() == zero
        s, t = sk.dummy_string(700), sk.dummy_string(5)                           # 2820 blocks: more than one chunk's worth
        assert sk.pool_stats() == dict(zero, live=2820) and sk.stats()["blocks_live"] == 2820
        tokens = _tokens(sk, t)
        for compact in (False, True):
            assert sk.pool_trim(compact=compact) == {"blocks_moved": 0, "bytes_released": 0}
            assert sk.pool_trim(compact=compact, keep_free_blocks=4096) == {"blocks_moved": 0, "bytes_released": 0}
        assert _tokens(sk, t) == tokens                                            # the planner's tokens are what they were
        del s
        assert sk.pool_stats() == dict(zero, live=20) and sk.stats()["blocks_live"] == 20
        sk.set_mode(1)
        r = sk.contains_clear(t, "ab")                                             # pending work: the trim flushes it
        assert sk.pool_trim() == {"blocks_moved": 0, "bytes_released": 0}
        assert sk.stats()["pbs_executed"] > 0 and sk.pool_stats()["live"] == sk.stats()["blocks_live"]
        del r, t
        assert sk.pool_stats() == zero
    finally:
        sk.close()


def _tokens(sk, s):
    """the block tokens of a string's characters (fhs_debug_char_terms: [kind 1, 0, 1, token, 1] per block)"""
    out = []
    for ch in s.chars:
        n = C.c_size_t()
        buf = np.zeros(64, np.uint64)
        sk.ctx._check(sk.ctx._L.fhs_debug_char_terms(sk.ctx._h, ch.h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)))
        words = buf[:n.value].reshape(4, 5)
        assert (words[:, 0] == 1).all()
        out += words[:, 3].tolist()
    return out


def test_levels_waiting_for_a_commit_refuse_the_trim(L):
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        sk.set_mode(1)
        sk.set_auto_flush(0)
        s = sk.dummy_string(6)
        r = sk.contains_clear(s, "ab")
        levels, width = C.c_uint64(), C.c_uint64()
        sk.ctx._check(L.fhs_flush_plan(sk.ctx._h, C.byref(levels), C.byref(width)))
        assert levels.value > 0
        moved = C.c_uint64(9)
        assert L.fhs_pool_trim(sk.ctx._h, 1, 0, C.byref(moved), None) == FHS_ERR_STATE and moved.value == 0
        assert "fhs_flush_level_commit" in L.fhs_last_error(sk.ctx._h).decode()
        assert L.fhs_pool_stats(sk.ctx._h, (C.c_uint64 * 6)()) == 0                # the figures are still there to read
        del r, s
    finally:
        sk.close()


def test_victim_choice(L):
    assert _plan(L, [CHUNK] * 3, 0) == [0, 0, 0]                                   # all full: no victim
    assert _plan(L, [CHUNK, 1, 0, 7], 0) == [0, 1, 1, 0]                           # 2056 live: chunk 0 and one more stay
    assert _plan(L, [5, 5, 5], 0) == [0, 1, 1]                                     # a tie goes to the later chunk
    assert _plan(L, [3, 9, 3, 9, 3], 6144 - 27) == [0, 0, 1, 0, 1]                 # ... among the emptiest only
    assert _plan(L, [CHUNK, 1, 0, 7], CHUNK) == [0, 0, 1, 0]                       # room for 2048 more: one chunk fewer goes
    assert _plan(L, [CHUNK, 1, 0, 7], CHUNK - 8) == [0, 1, 1, 0]                   # 2056 + 2040 fit two chunks exactly
    assert _plan(L, [CHUNK, 1, 0, 7], CHUNK - 7) == [0, 0, 1, 0]                   # ... one block more does not
    assert _plan(L, [0, 0, 0], 0) == [1, 1, 1]                                     # nothing live, nothing kept
    assert _plan(L, [0, 0, 0], 1) == [0, 1, 1]
    assert _plan(L, [1, 0], 10 ** 18) == [0, 0] and _plan(L, [1, 0], 2 ** 64 - 1) == [0, 0]   # no sum wraps
    assert _plan(L, [], 0) == []
    rng = np.random.default_rng(18)                                               # the rule, restated, on random occupancies
    for _ in range(50):
        n = int(rng.integers(1, 12))
        live = rng.integers(0, CHUNK + 1, n) * (rng.random(n) < 0.7)
        keep = int(rng.integers(0, 3 * CHUNK))
        k = -(-(int(live.sum()) + keep) // CHUNK)
        order = sorted(range(n), key=lambda i: (live[i], -i))
        want = [0] * n
        for i in order[:max(n - k, 0)]:
            want[i] = 1
        assert _plan(L, live, keep) == want, (live.tolist(), keep)


def test_bindings_are_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(ROOT, "bindings", "fhestring_hip.rs")).read()
    for name in ("fhs_pool_stats", "fhs_pool_trim", "fhs_debug_pool_plan", "FHS_TRIM_RELEASE", "FHS_TRIM_COMPACT"):
        assert name in text, name
