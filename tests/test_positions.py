"""char_at / substr / take / skip / split_at / slice: encrypted positions (the u8 of find / rfind / len, the (lo, hi) pair
of their _wide forms) as operands.  The reference has no such method; the semantics are stated
here in Python on the buffer's bytes, NULs included:

    char_at(s, p)       = buf[p] if p < n else 0
    substr(s, p, count) = [buf[p + j] if p + j < n else 0 for j < count]
    take(s, p)          = [buf[j] if j < p else 0 for j < n]
    split_at(s, p)      = (take(s, p), substr(s, p, n))

All on the CPU:

* the logic by constant folding on a planner context, fused and as written, the two against each other;
* composition with find_clear / find_clear_wide, an absent position included;
* the bookkeeping on uploaded inputs: noise budget, result noise, depth, growth with n, what a trivial and an int
  position record, the pinned figures of tests/golden/positions_plan.json (tools/gen_positions_plan.py), and that find /
  rfind / len record what they recorded;
* real ciphertexts through the CPU oracle's bootstrap (oracle/plan_exec.py);
* the edges of the C ABI."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import strings as ostr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_positions_plan as gen  # noqa: E402

BUDGET = 64
NAMES = ("fhs_str_char_at", "fhs_str_char_at_wide", "fhs_str_substr", "fhs_str_substr_wide", "fhs_str_take",
         "fhs_str_take_wide", "fhs_str_split_at", "fhs_str_split_at_wide")


@pytest.fixture(scope="module")
def folded():
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    yield sk
    sk.close()


@pytest.fixture()
def planner():
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    sk.set_mode(1)
    sk.set_auto_flush(0)
    yield sk
    sk.close()


def _triv(sk, data):
    from fhestring_amd.api import FheString
    return FheString([sk.trivial(b) for b in data])


def _pos(sk, p, wide):
    from fhestring_amd.api import FheU16
    return FheU16(sk.trivial(p & 255), sk.trivial(p >> 8)) if wide else sk.trivial(p)


def _bytes(s):
    out = [c.trivial_value() for c in s]
    assert None not in out, "the result did not fold to constants"
    return bytes(out)


def _buffer(n):
    """letters with a NUL at every seventh place from 3 on: NULs in the middle, nothing is compacted"""
    return bytes(0 if i % 7 == 3 else 0x41 + i % 26 for i in range(n))


# ---- the semantics, in Python ---------------------------------------------------------------------------------------
def py_substr(buf, p, count):
    return bytes(buf[p + j] if p + j < len(buf) else 0 for j in range(count))


def py_take(buf, p):
    return bytes(buf[j] if j < p else 0 for j in range(len(buf)))


def _all_ops(sk, s, pos, counts):
    """every operation on (s, pos): a dict of byte strings"""
    got = {"char_at": bytes([sk.char_at(s, pos).trivial_value()]), "take": _bytes(sk.take(s, pos))}
    for c in counts:
        got["substr%d" % c] = _bytes(sk.substr(s, pos, c))
    head, tail = sk.split_at(s, pos)
    got["split_at"] = _bytes(head) + b"|" + _bytes(tail)
    return got


def _all_want(buf, p, counts):
    want = {"char_at": py_substr(buf, p, 1), "take": py_take(buf, p)}
    for c in counts:
        want["substr%d" % c] = py_substr(buf, p, c)
    want["split_at"] = py_take(buf, p) + b"|" + py_substr(buf, p, len(buf))
    return want


# ---- 1. folding against Python --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 21, 64, 65, 255, 256, 257, 300])
def test_u8_positions_fold_to_python(folded, n):
    sk = folded
    buf = _buffer(n)
    s = _triv(sk, buf)
    positions = sorted(p for p in {0, 1, 2, 3, 4, 15, 16, 63, 64, n - 2, n - 1, n, n + 1, 254, 255} if 0 <= p <= 255)
    for p in positions:
        sk.set_mode(1)
        counts = sorted({1, 3, n, n + 5})
        fused = _all_ops(sk, s, _pos(sk, p, False), counts)
        assert fused == _all_want(buf, p, counts), (n, p)
        if n <= 64:                                          # as written: the independent statement of the semantics
            sk.set_mode(0)
            small = [c for c in counts if c <= 8]
            written = _all_ops(sk, s, _pos(sk, p, False), small)
            assert written == _all_want(buf, p, small), (n, p)
            assert all(written[k] == fused[k] for k in written), (n, p)
    assert sk.stats(reset=True)["pbs_executed"] == 0         # everything folded


@pytest.mark.parametrize("n", [300, 1030])
def test_wide_positions_fold_to_python(folded, n):
    sk = folded
    sk.set_mode(1)
    buf = _buffer(n)
    s = _triv(sk, buf)
    for p in (0, 255, 256, 257, 1023, 1024, n - 1, n, 4096, 65535):
        counts = (1, 3, n, n + 5)
        assert _all_ops(sk, s, _pos(sk, p, True), counts) == _all_want(buf, p, counts), (n, p)
    if n == 300:                                             # a u8 position on a long buffer is taken literally
        for p in (0, 254, 255):
            assert _all_ops(sk, s, _pos(sk, p, False), (3, n)) == _all_want(buf, p, (3, n)), p
        sk.set_mode(0)
        for p in (0, 257, 299, 300, 65535):
            assert sk.char_at(s, _pos(sk, p, True)).trivial_value() == py_substr(buf, p, 1)[0], p
        sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0


def test_wide_as_written_agrees_on_a_short_buffer(folded):
    sk = folded
    buf = _buffer(21)
    s = _triv(sk, buf)
    for p in (0, 3, 20, 21, 255, 256, 65535):
        got = {}
        for mode in (0, 1):
            sk.set_mode(mode)
            got[mode] = _all_ops(sk, s, _pos(sk, p, True), (1, 5))
        assert got[0] == got[1] == _all_want(buf, p, (1, 5)), p
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0


def test_int_positions_and_the_derived_methods(folded):
    sk = folded
    sk.set_mode(1)
    buf = _buffer(21)
    s = _triv(sk, buf)
    for p in (0, 5, 20, 21, 40):
        assert sk.char_at(s, p).trivial_value() == py_substr(buf, p, 1)[0]
        assert _bytes(sk.substr(s, p, 6)) == py_substr(buf, p, 6)
        assert _bytes(sk.take(s, p)) == py_take(buf, p)
        assert _bytes(sk.skip(s, p)) == py_substr(buf, p, 21) == _bytes(sk.skip(s, _pos(sk, p, False)))
        head, tail = sk.split_at(s, p)
        assert (_bytes(head), _bytes(tail)) == (py_take(buf, p), py_substr(buf, p, 21))
    for a, b in ((0, 21), (2, 9), (9, 2), (5, 40), (30, 40)):
        want = (buf[a:b] + bytes(21))[:21]
        assert _bytes(sk.slice(s, a, b)) == want
        assert _bytes(sk.slice(s, _pos(sk, a, False), _pos(sk, b, True))) == want
    assert sk.stats(reset=True)["pbs_executed"] == 0


# ---- 2. composition, folded ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["as_written", "fused"])
def test_substr_of_find_spells_the_pattern(folded, mode):
    sk = folded
    sk.set_mode(mode)
    text, pat = "the quick brown fox", "brown"
    buf = ostr.pad_plain(text, 3)
    s = _triv(sk, buf)
    pos = sk.find_clear(s, pat)
    assert pos.trivial_value() == text.find(pat)
    assert _bytes(sk.substr(s, pos, len(pat))) == pat.encode()
    assert sk.char_at(s, pos).trivial_value() == ord("b")
    assert _bytes(sk.take(s, pos)).rstrip(b"\0") == b"the quick "
    head, tail = sk.split_at(s, pos)
    assert (_bytes(head).rstrip(b"\0"), _bytes(tail).rstrip(b"\0")) == (b"the quick ", b"brown fox")
    miss = sk.find_clear(s, "zebra")
    assert miss.trivial_value() == 255
    assert _bytes(sk.substr(s, miss, 5)) == bytes(5) and sk.char_at(s, miss).trivial_value() == 0
    assert _bytes(sk.take(s, miss)) == bytes(buf)
    head, tail = sk.split_at(s, miss)
    assert (_bytes(head), _bytes(tail)) == (bytes(buf), bytes(len(buf)))
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0


def test_substr_of_find_wide_spells_the_pattern(folded):
    sk = folded
    sk.set_mode(1)
    pat = "Qz7#"
    text = ("abcdefghijklmnopqrstuvwxy" * 12)[:300]
    text = text[:257] + pat + text[257 + len(pat):]
    buf = ostr.pad_plain(text, 1)
    s = _triv(sk, buf)
    pos = sk.find_clear_wide(s, pat)
    assert pos.trivial_value() == 257
    assert _bytes(sk.substr(s, pos, len(pat))) == pat.encode() and sk.char_at(s, pos).trivial_value() == ord("Q")
    assert _bytes(sk.take(s, pos)) == py_take(bytes(buf), 257)
    miss = sk.find_clear_wide(s, "Qz7!")
    assert miss.trivial_value() == 65535
    assert _bytes(sk.substr(s, miss, 4)) == bytes(4) and _bytes(sk.take(s, miss)) == bytes(buf)
    head, tail = sk.split_at(s, miss)
    assert (_bytes(head), _bytes(tail)) == (bytes(buf), bytes(len(buf)))
    assert sk.stats(reset=True)["pbs_executed"] == 0


# ---- 3. bookkeeping on uploaded inputs (fused) --------------------------------------------------------------------------
def _flush_stats(sk, fn):
    sk.flush()
    sk.stats(reset=True)
    keep = fn()
    sk.flush()
    return sk.stats(), sk.level_widths(), keep


def _chars_of(result):
    from fhestring_amd.api import FheAsciiChar
    if isinstance(result, FheAsciiChar):
        return [result]
    if isinstance(result, tuple):
        return [c for part in result for c in part]
    return list(result)


def _bits(n, wide):
    k = 0
    while (1 << k) < n and k < (16 if wide else 8):
        k += 1
    return k


def _check_op(sk, n, wide, make_pos, extra_levels=0):
    """every operation on a fresh uploaded string of n characters and the position make_pos(s) hands over"""
    s = sk.dummy_string(n)
    for op in ("char_at", "substr_8", "substr_n", "take", "split_at"):
        st, _, res = _flush_stats(sk, lambda: gen.run_op(sk, op, s, make_pos(s)))
        assert 0 < st["max_input_sum_c2"] <= BUDGET, (op, n, st)
        assert st["levels"] <= _bits(n, wide) + 4 + extra_levels, (op, n, st["levels"])
        for ch in _chars_of(res):
            assert ch.trivial_value() is not None or ch.sum_c2() <= 4, (op, n, ch.sum_c2())


@pytest.mark.parametrize("n", [21, 256, 300])
def test_budget_depth_and_result_noise_u8(planner, n):
    p = planner.dummy_string(1)[0]
    _check_op(planner, n, False, lambda s: p)


def test_budget_depth_and_result_noise_wide(planner):
    from fhestring_amd.api import FheU16
    p = planner.dummy_string(2)
    _check_op(planner, 1030, True, lambda s: FheU16(p[0], p[1]))


def test_budget_with_the_position_of_a_real_find(planner):
    """find's digits come back as sums of up to 57 bootstrap outputs: they are refreshed on the way in.  find and its
    consumer are one DAG here, as a caller records them: the depth is find's (6 levels at these sizes, tests/
    test_planner.py) and the refresh on top of the consumer's."""
    sk = planner
    pat4, pat2 = sk.dummy_string(4), sk.dummy_string(2)
    seen = []

    def wide(s):
        pos = sk.find_wide(s, pat4)
        seen.append(max(pos.lo.sum_c2(), pos.hi.sum_c2()))
        return pos

    def narrow(s):
        pos = sk.find(s, pat2)
        seen.append(pos.sum_c2())
        return pos

    _check_op(sk, 300, True, wide, extra_levels=6)
    _check_op(sk, 21, False, narrow, extra_levels=6)
    assert min(seen) > 4 and max(seen) <= 57, seen


def test_cost_grows_as_designed():
    """executed + extracted bootstraps at 512 against 256 characters: n log n gives 2.2, a quadratic design 4, linear 2."""
    from fhestring_amd.api import MyServerKey
    cost = {}
    for op in ("substr_n", "char_at", "take"):
        for n in (256, 512):
            sk = MyServerKey.planner()
            try:
                r = gen.measure(sk, op, n)
            finally:
                sk.close()
            cost[op, n] = r["pbs_executed"] + r["pbs_extracted"]
    assert cost["substr_n", 512] <= 2.4 * cost["substr_n", 256], cost
    assert cost["char_at", 512] <= 2.2 * cost["char_at", 256], cost
    assert cost["take", 512] <= 2.2 * cost["take", 256], cost
    for n in (256, 512):
        assert cost["char_at", n] < cost["substr_n", n], cost


def test_trivial_and_int_positions_record_nothing(planner):
    """A trivial position folds every bit, every flag of the thermometer and the overflow flag: the shift becomes a
    static one, and since no block gains noise the construction's closing refresh (done only above sum c^2 = 4) does not
    happen either -- no bootstrap at all on an uploaded string, and the operand's own blocks come back."""
    sk = planner
    s = sk.dummy_string(21)
    sk.flush()
    st0 = sk.stats(reset=True)
    for p in (0, 7, 20, 21, 255):
        for wide in (False, True):
            res = [sk.char_at(s, _pos(sk, p, wide)), sk.substr(s, _pos(sk, p, wide), 5), sk.take(s, _pos(sk, p, wide)),
                   sk.split_at(s, _pos(sk, p, wide))]
            sk.flush()
            del res
    st = sk.stats()
    assert (st["pbs_executed"], st["pbs_extracted"], st["levels"]) == (0, 0, 0), st
    sk.stats(reset=True)
    before = sk.stats()
    res = [sk.char_at(s, 3), sk.substr(s, 3, 5), sk.take(s, 3), sk.skip(s, 3), sk.split_at(s, 3), sk.slice(s, 2, 9)]
    sk.flush()
    after = sk.stats()
    del res
    assert {k: after[k] for k in ("pbs_executed", "pbs_folded", "pbs_shared", "levels")} == \
        {k: before[k] for k in ("pbs_executed", "pbs_folded", "pbs_shared", "levels")}
    assert st0["pbs_executed"] == 0


def test_pinned_plan():
    """The figures of tests/golden/positions_plan.json (DESIGN section 19 quotes them): a change there is a change of the
    DAG."""
    from fhestring_amd.api import MyServerKey
    with open(gen.PATH) as f:
        pinned = json.load(f)
    for ops, sizes in ((gen.NARROW_OPS, gen.NARROW_SIZES), (gen.WIDE_OPS, gen.WIDE_SIZES)):
        for op in ops:
            for n in sizes:
                sk = MyServerKey.planner()
                try:
                    got = gen.measure(sk, op, n)
                finally:
                    sk.close()
                assert got == pinned["ops"][op][str(n)], (op, n)
                assert got["pbs_executed"] > 0 and got["max_input_sum_c2"] <= BUDGET


def test_find_rfind_len_record_what_they_recorded(planner):
    sk = planner
    s, pat, p = sk.dummy_string(257), sk.dummy_string(4), sk.dummy_string(1)[0]
    probes = (lambda: sk.find(s, pat), lambda: sk.rfind(s[:250], pat), lambda: sk.len(s))
    before = [_flush_stats(sk, f)[:2] for f in probes]
    assert (before[0][0]["pbs_executed"], before[0][0]["levels"]) == (2574, 6)    # config 3's find: tests/test_planner.py
    keep = (sk.char_at(s, p), sk.substr(s, p, 8), sk.take(s, p), sk.split_at(s, p))
    sk.flush()
    del keep
    after = [_flush_stats(sk, f)[:2] for f in probes]
    assert before == after


# ---- 4. real ciphertexts, the CPU oracle's bootstrap -----------------------------------------------------------------
def test_results_decrypt_on_real_ciphertexts(oracle_keys, oracle_sk):
    from oracle.plan_exec import PlanRun
    K = oracle_keys
    run = PlanRun(oracle_sk, threads=min(16, os.cpu_count() or 1), mode=6)
    try:
        sk = run.sk
        text = "the quick brown fox"
        buf = bytes(ostr.pad_plain(text, 24 - len(text)))
        assert len(buf) == 24
        s = run.upload_string(np.stack([K.encrypt_char(b) for b in buf]))
        outs = {}
        for name, pat in (("hit", "brown"), ("miss", "zebra")):
            pos = sk.find_clear(s, pat)
            outs[name] = (sk.substr(s, pos, 5), sk.char_at(s, pos), sk.take(s, pos))
        filler = ("abcdefghijklmnopqrstuvwxy" * 11)[:260]
        long_text = filler[:257] + "Q" + filler[258:]            # one character: the cheapest find that lands past 255
        w = run.upload_string(np.stack([K.encrypt_char(b) for b in long_text.encode()]))
        outs["wide"] = sk.char_at(w, sk.find_clear_wide(w, "Q"))
        run.run()
        st = sk.stats()
        dec = lambda ch: K.decrypt_char(run.result_char(ch))
        dec_s = lambda chars: bytes(dec(ch) for ch in chars)
        for name, p in (("hit", text.find("brown")), ("miss", 255)):
            sub, ch, head = outs[name]
            assert dec_s(sub) == py_substr(buf, p, 5), name
            assert dec(ch) == py_substr(buf, p, 1)[0], name
            assert dec_s(head) == py_take(buf, p), name
        assert dec_s(outs["hit"][0]) == b"brown"
        assert dec(outs["wide"]) == ord("Q") and long_text.find("Q") == 257
        assert st["max_input_sum_c2"] <= BUDGET and 1000 < run.pbs < 5000, run.pbs
    finally:
        run.close()


# ---- 5. the edges of the C ABI -----------------------------------------------------------------------------------------
def test_names_prototypes_and_the_rust_binding(planner):
    from fhestring_amd import cabi
    names = {f[0] for f in cabi.parse_header()["funcs"]}
    assert set(NAMES) <= names
    for n in NAMES:
        assert getattr(planner.ctx._L, n).argtypes is not None
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(ROOT, "bindings", "fhestring_hip.rs")).read()
    for n in NAMES:
        assert "fn %s(" % n in text, n


def _calls(L, h, s, n, pos, out, out2, count=3):
    """every entry point with (s, n), a position handle for both halves, and the outputs given"""
    return [("char_at", lambda: L.fhs_str_char_at(h, s, n, pos, out)),
            ("char_at_wide", lambda: L.fhs_str_char_at_wide(h, s, n, pos, pos, out)),
            ("substr", lambda: L.fhs_str_substr(h, s, n, pos, count, out)),
            ("substr_wide", lambda: L.fhs_str_substr_wide(h, s, n, pos, pos, count, out)),
            ("take", lambda: L.fhs_str_take(h, s, n, pos, out)),
            ("take_wide", lambda: L.fhs_str_take_wide(h, s, n, pos, pos, out)),
            ("split_at", lambda: L.fhs_str_split_at(h, s, n, pos, out, out2)),
            ("split_at_wide", lambda: L.fhs_str_split_at_wide(h, s, n, pos, pos, out, out2))]


def test_argument_errors_record_nothing(planner):
    from fhestring_amd.api import _harr
    sk = planner
    L, h = sk.ctx._L, sk.ctx._h
    s = sk.dummy_string(5)
    pos = sk.dummy_string(1)[0]
    gone = sk.dummy_string(1)[0]
    released = gone.h
    del gone                                                 # a handle that was valid once
    sk.flush()
    st0 = sk.stats()
    arr, out, out2 = _harr(s.chars), (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
    bad_s = (C.c_uint64 * 5)(*[c.h for c in s.chars[:4]], released)
    ERR_ARG = -1
    for name, call in _calls(L, None, arr, 5, pos.h, out, out2):                     # a null context
        assert call() == ERR_ARG, name
    for name, call in _calls(L, h, arr, 5, pos.h, None, out2) + _calls(L, h, arr, 5, pos.h, out, None)[6:]:   # a null output
        assert call() == ERR_ARG, name
    for name, call in _calls(L, h, arr, 5, released, out, out2) + _calls(L, h, arr, 5, 0, out, out2):   # the position
        assert call() == ERR_ARG, name
    for name, call in _calls(L, h, bad_s, 5, pos.h, out, out2) + _calls(L, h, None, 5, pos.h, out, out2):   # the string
        assert call() == ERR_ARG, name
    sk.flush()
    assert sk.stats() == st0                                 # no node, no bootstrap, no block


def test_empty_operand_and_empty_request(planner):
    from fhestring_amd.api import FheAsciiChar, FheU16, _harr
    sk = planner
    L, h = sk.ctx._L, sk.ctx._h
    s = sk.dummy_string(5)
    noisy = sk.find(s, sk.dummy_string(2))                   # its digits would be refreshed if it were loaded
    sk.flush()
    assert noisy.sum_c2() > 4
    st0 = sk.stats()
    for pos in (noisy, FheU16(noisy, noisy)):
        assert sk.char_at([], pos).trivial_value() == 0                           # n = 0: NULs
        assert _bytes(sk.substr([], pos, 3)) == bytes(3)
        assert len(sk.take([], pos)) == 0 and [len(x) for x in sk.split_at([], pos)] == [0, 0]
        assert len(sk.substr(s, pos, 0)) == 0                                       # count = 0: nothing
    arr = _harr(s.chars)
    assert L.fhs_str_substr(h, arr, 5, noisy.h, 0, None) == 0                      # ... and needs no output
    assert L.fhs_str_substr_wide(h, arr, 5, noisy.h, noisy.h, 0, None) == 0
    assert L.fhs_str_take(h, None, 0, noisy.h, None) == 0
    assert L.fhs_str_split_at_wide(h, None, 0, noisy.h, noisy.h, None, None) == 0
    out = (C.c_uint64 * 1)()
    assert L.fhs_str_char_at(h, None, 0, noisy.h, out) == 0
    assert FheAsciiChar(sk, out[0]).trivial_value() == 0
    sk.flush()
    assert sk.stats() == st0
