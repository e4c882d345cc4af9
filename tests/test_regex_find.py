"""regex_find_clear / regex_find_clear_wide / regex_starts_clear: where a match of a clear regular expression starts
(DESIGN.md section 25).  The reference has no such method; the semantics are Python's own, on text = the buffer up to its
first NUL, with rx = re.compile(pattern, re.S | (re.I if ignore_case else 0)):

    starts[i] = i <= len(text) and rx.match(text, i) is not None          find = rx.search(text).start(), or absent

All on the CPU, after tests/test_regex.py, whose patterns, buffers and random generator are imported unmodified:

* the logic by constant folding on a planner context, fused and as written, against `re` and against each other: the
  fixed patterns on buffers of seven sizes, chosen cases, and a seeded random sweep whose make-up is asserted;
* the bookkeeping on uploaded inputs: the noise budget, the flags' noise, the depth bound against find_class's, literals
  without tables, the tables of the plan, composition with substr, and the pinned figures of
  tests/golden/regex_find_plan.json (tools/gen_regex_find_plan.py);
* real ciphertexts through the CPU oracle's bootstrap (oracle/plan_exec.py);
* the edges of the C ABI."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_regex_find_plan as gen  # noqa: E402
from test_regex import FIXED, SEARCHES, TEXT, _buffers, _random_case  # noqa: E402

BUDGET = 64
ERR_ARG, ERR_LIMIT = -1, -4
ABSENT, WIDE_ABSENT = 255, 65535
SEARCH_BIT = 2                                                # FHS_REGEX_SEARCH


def _rx(pattern, ignore_case=False):
    return re.compile(pattern, re.S | (re.I if ignore_case else 0))


def py_starts(buf, pattern, ignore_case=False):
    text, rx = bytes(buf).split(b"\0")[0], _rx(pattern, ignore_case)
    return [int(i <= len(text) and rx.match(text, i) is not None) for i in range(len(buf))]


def py_find(buf, pattern, ignore_case=False, absent=ABSENT):
    m = _rx(pattern, ignore_case).search(bytes(buf).split(b"\0")[0])
    return m.start() if m else absent


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


def _both_modes(sk, s, buf, pattern, ignore_case=False):
    """all three calls in both modes on a trivially encrypted string: (find, starts), checked against Python, against
    each other and against one another's meaning (find is the first set flag)"""
    want_starts, want = py_starts(buf, pattern, ignore_case), py_find(buf, pattern, ignore_case)
    if len(buf):                                             # (no character, no flag: the empty match at 0 has none to set)
        assert want == (want_starts.index(1) if 1 in want_starts else ABSENT)
    for mode in (1, 0):
        sk.set_mode(mode)
        starts = [c.trivial_value() for c in sk.regex_starts_clear(s, pattern, ignore_case=ignore_case)]
        find = sk.regex_find_clear(s, pattern, ignore_case=ignore_case).trivial_value()
        wide = sk.regex_find_clear_wide(s, pattern, ignore_case=ignore_case).trivial_value()
        what = (bytes(buf), pattern, ignore_case, mode)
        assert starts == want_starts, (what, starts, want_starts)
        assert find == want and wide == (want if want != ABSENT else WIDE_ABSENT), (what, find, wide, want)
    return want, want_starts


# ---- 1. folding against Python ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 5, 16, 17, 64])
def test_fixed_patterns_fold_to_python(folded, n):
    sk = folded
    for buf in _buffers(n):
        assert len(buf) == n
        s = _triv(sk, buf)
        for pattern in FIXED + SEARCHES:
            for ignore_case in (False, True):
                _both_modes(sk, s, buf, pattern, ignore_case)
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0         # everything folded


# ---- 2. chosen cases --------------------------------------------------------------------------------------------------
def test_positions_and_the_first_nul(folded):
    """a match at 0, in the middle, ending at the last text character, only beyond the first NUL, and across it"""
    sk = folded
    buf = b"start middle end\0beyond\0"
    s = _triv(sk, buf)
    got = [_both_modes(sk, s, buf, p)[0] for p in (b"start", b"mid+le", b"end", b"beyond", rb"d\0b", b"e[a-z]d", b"e[a-z]{2}d")]
    assert got == [0, 6, 13, ABSENT, ABSENT, 13, ABSENT]
    assert _both_modes(sk, s, buf, b"START", ignore_case=True)[0] == 0 and _both_modes(sk, s, buf, b"START")[0] == ABSENT


def test_leftmost_start_whatever_the_branch_order(folded):
    sk = folded
    assert _both_modes(sk, _triv(sk, b"xabab"), b"xabab", b"b|ab")[0] == 1
    assert _both_modes(sk, _triv(sk, b"zabcd"), b"zabcd", b"(a|ab)(c|bcd)")[0] == 1


def test_nullable_patterns(folded):
    sk = folded
    for buf in (b"\0ab", b"\0\0\0", b"\0"):
        for pattern in (b"", b"a*", b"(ab|cd)*e?"):
            assert _both_modes(sk, _triv(sk, buf), buf, pattern) == (0, [1] + [0] * (len(buf) - 1))
    assert _both_modes(sk, _triv(sk, b"ba\0a"), b"ba\0a", b"a*")[1] == [1, 1, 1, 0]
    assert _both_modes(sk, _triv(sk, b""), b"", b"a*") == (0, []) and _both_modes(sk, _triv(sk, b""), b"", b"a") == (ABSENT, [])


# ---- 3. the random sweep ----------------------------------------------------------------------------------------------
def test_random_sweep_folds_to_python(folded):
    sk = folded
    rng = random.Random(24)
    later = absent = beyond_only = flags = flags_set = 0
    for _ in range(2400):
        buf, pattern, ignore_case, _search = _random_case(rng)
        buf = bytes(rng.choice(b"xy") for _ in range(rng.randint(0, 5))) + buf     # or almost every match starts at 0
        want, want_starts = _both_modes(sk, _triv(sk, buf), buf, pattern, ignore_case)
        later += 0 < want < ABSENT
        absent += want == ABSENT
        beyond_only += want == ABSENT and any(_rx(pattern, ignore_case).search(part) for part in buf.split(b"\0")[1:])
        if _rx(pattern).match(b"") is None:                  # not nullable
            flags += len(buf)
            flags_set += sum(want_starts)
    # judged by `re` alone: a later edit of the generator cannot hollow the sweep out
    assert later >= 400 and absent >= 400 and beyond_only >= 25, (later, absent, beyond_only)
    assert 0.10 * flags <= flags_set <= 0.40 * flags, (flags_set, flags)
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0


# ---- 4. bookkeeping on uploaded inputs (fused) ------------------------------------------------------------------------
def _flush_stats(sk, fn):
    sk.flush()
    sk.stats(reset=True)
    keep = fn()
    sk.flush()
    return sk.stats(), sk.level_widths(), keep


# A step holds w * |in| + k <= 15 with k flags to OR, w = k + 1, within the noise budget; more go
# through or_tree first, one more level.  Backwards the k flags are a position's FOLLOWERS, and only for a position that
# is not a last one itself (a last position needs no follower: its step folds to its class test).  In FIXED + SEARCHES no
# cycle has such a position with too many followers: in `(A|B|-|2|0|4| |e)+.*`, test_regex.py's case, every position is
# a last one, and the nine followers of `[A-Z]` in `[A-Z](a|...|B)[-x].*` and the eight first positions of the former
# cost one level once, at the front, inside the slack.
# The mirror image of test_regex.py's case does it at EVERY index: each branch is followed by the eight and `x`, 2 * 10 + 9.
OR_AT_EVERY_INDEX = (b".*(A|B|-|2|0|4| |e)+x",)


@pytest.mark.parametrize("n", [17, 64])
def test_budget_flag_noise_and_depth(planner, n):
    sk = planner
    s = sk.dummy_string(n)
    find_levels = _flush_stats(sk, lambda: sk.find_class(s, "a-z"))[0]["levels"]      # the same f_find_digits tail
    simple = 2 + n + 1 + find_levels                         # class tests, one step per character, the start step, the tail
    recorded = 0
    for pattern in FIXED + SEARCHES + list(OR_AT_EVERY_INDEX):
        for ignore_case in (False, True):
            st, w, res = _flush_stats(sk, lambda: sk.regex_find_clear(s, pattern, ignore_case=ignore_case))
            if res.trivial_value() is not None:              # decided by the pattern alone
                assert st["pbs_executed"] == 0, pattern
            else:
                recorded += 1
                assert 0 < st["max_input_sum_c2"] <= BUDGET, (pattern, ignore_case, st)
                assert st["levels"] == len(w)
                assert st["levels"] <= simple + (n if pattern in OR_AT_EVERY_INDEX else 0), (pattern, ignore_case, st["levels"], simple)
                if pattern in OR_AT_EVERY_INDEX:
                    assert st["levels"] > simple             # the or_tree path was taken
            del res
            st, w, flags = _flush_stats(sk, lambda: sk.regex_starts_clear(s, pattern, ignore_case=ignore_case))
            assert st["max_input_sum_c2"] <= BUDGET, (pattern, ignore_case, st)
            for f in flags:
                assert f.sum_c2() == (0 if f.trivial_value() is not None else 1), (pattern, ignore_case, f.sum_c2())
            del flags
    assert recorded >= 100


def test_trivial_decisions_load_nothing(planner):
    sk = planner
    s = sk.dummy_string(5)
    noisy = sk.find(s, sk.dummy_string(2))                   # its digits would be refreshed if it were loaded
    sk.flush()
    assert noisy.sum_c2() > 4
    st0 = sk.stats()
    chars = s.chars + [noisy]
    for mode in (0, 1):
        sk.set_mode(mode)
        for pattern in ("a*", "", "(ab|cd)*e?"):             # nullable: the empty match at 0
            assert sk.regex_find_clear(chars, pattern).trivial_value() == 0
            assert sk.regex_find_clear_wide(chars, pattern).trivial_value() == 0
            assert sk.regex_find_clear([], pattern).trivial_value() == 0 and len(sk.regex_starts_clear([], pattern)) == 0
        for pattern in (".{7}", "abcdefg"):                  # the shortest match is longer than the buffer
            assert sk.regex_find_clear(chars, pattern).trivial_value() == ABSENT
            assert sk.regex_find_clear_wide(chars, pattern).trivial_value() == WIDE_ABSENT
            assert [f.trivial_value() for f in sk.regex_starts_clear(chars, pattern)] == [0] * 6
        assert sk.regex_find_clear([], "a").trivial_value() == ABSENT and len(sk.regex_starts_clear([], "a")) == 0
    sk.set_mode(1)
    sk.flush()
    assert sk.stats() == st0                                 # no node, no bootstrap, no refresh of the noisy operand
    flags = sk.regex_starts_clear(chars, "a*")               # the flags of a nullable pattern do depend on the string
    assert flags[0].trivial_value() == 1 and flags[1].trivial_value() is None


@pytest.mark.parametrize("pattern", ["abc", "error: timeout"])
def test_a_literal_pattern_needs_no_table(planner, pattern):
    from fhestring_amd import lib
    sk = planner
    luts0 = lib().fhs_user_lut_count()
    for n in (17, 64):
        for call in (sk.regex_find_clear, sk.regex_starts_clear):
            s = sk.dummy_string(n)
            _, w, res = _flush_stats(sk, lambda: call(s, pattern))
            assert w[0] <= 2 * n + n, (n, w)                 # two nibble rotations per character, and the zero tests
            del res, s
            s = sk.dummy_string(n)
            _, w2, res = _flush_stats(sk, lambda: call(s, pattern, ignore_case=True))
            assert w2[0] <= w[0]                             # the other case rides along as an extraction
            del res, s
    assert lib().fhs_user_lut_count() == luts0


def test_threshold_tables_are_registered_with_the_plan(planner):
    """the class (one no other test writes: the registry is process-wide and interned) has four followers; on two characters only `y` can follow it, on nine all four can: the tables are the same"""
    from fhestring_amd import lib
    sk = planner
    count = lib().fhs_user_lut_count
    before = count()
    res = sk.regex_find_clear(sk.dummy_string(2), r"[\x03q-s\x7f%](t|u|v)*y")
    after_short = count()
    assert after_short > before and res.trivial_value() is None
    del res
    res = sk.regex_find_clear(sk.dummy_string(9), r"[\x03q-s\x7f%](t|u|v)*y")
    flags = sk.regex_starts_clear(sk.dummy_string(9), r"[\x03q-s\x7f%](t|u|v)*y")
    assert count() == after_short
    del res, flags


def test_as_written_registers_no_table(planner):
    from fhestring_amd import lib
    sk = planner
    s = sk.dummy_string(4)
    sk.set_mode(0)
    luts0 = lib().fhs_user_lut_count()
    for pattern in ("[b-y]+", "[q-t8]x", "(a|b|c)[d-g]", r"[^\W_]+z"):
        res = (sk.regex_find_clear(s, pattern), sk.regex_find_clear_wide(s, pattern), sk.regex_starts_clear(s, pattern))
        assert res[0].trivial_value() is None
        del res
    assert lib().fhs_user_lut_count() == luts0
    sk.set_mode(1)
    res = sk.regex_find_clear(s, "[q-t8]x")                   # the same class, fused: its tables
    assert lib().fhs_user_lut_count() > luts0
    del res


def test_composition_with_substr(folded):
    """section 19's consumers take the position: the four characters from the first digit run"""
    sk = folded
    buf = TEXT[:32] + bytes(4)
    s = _triv(sk, buf)
    at = re.search(rb"[0-9]+", buf).start()
    assert at == 3
    for mode in (1, 0):
        sk.set_mode(mode)
        for find in (sk.regex_find_clear, sk.regex_find_clear_wide):
            cut = sk.substr(s, find(s, "[0-9]+"), 4)
            assert bytes(c.trivial_value() for c in cut) == buf[at:at + 4] == b"2024"
            cut = sk.substr(s, find(s, "[0-9]{5}"), 4)        # absent: past the end
            assert bytes(c.trivial_value() for c in cut) == bytes(4)
    sk.set_mode(1)


# ---- 5. pinned figures ------------------------------------------------------------------------------------------------
def test_pinned_plan():
    """The figures of tests/golden/regex_find_plan.json (DESIGN section 25 quotes them): a change there is a change of the DAG."""
    with open(gen.PATH) as f:
        pinned = json.load(f)
    assert len(gen.CASES) == 25 and sorted(pinned["cases"]) == sorted(gen.key(*c) for c in gen.CASES)
    for case in gen.CASES:
        got = gen.measure_find(*case)
        assert got == pinned["cases"][gen.key(*case)], case
        assert got["max_input_sum_c2"] <= BUDGET and got["levels"] == len(got["level_widths"])
        assert (got["pbs_executed"] > 0) == (case[:2] != ("find", "(ab|cd)*e?")), case      # nullable: a trivial 0


# ---- 6. real ciphertexts, the CPU oracle's bootstrap ------------------------------------------------------------------
def test_results_decrypt_on_real_ciphertexts(oracle_keys, oracle_sk):
    from oracle.plan_exec import PlanRun
    K = oracle_keys
    run = PlanRun(oracle_sk, threads=min(16, os.cpu_count() or 1), mode=6)
    try:
        sk = run.sk
        buf = b"zama!\0"
        s = run.upload_string(np.stack([K.encrypt_char(b) for b in buf]))
        cases = [("ma", {}), ("[a-z]!", {}), ("z(am)*a!", {}), ("M[AB]!", {"ignore_case": True}), ("x", {}),
                 ("(z|a|m)+[ -/]", {})]
        outs = [sk.regex_find_clear(s, p, **kw) for p, kw in cases]
        flags = sk.regex_starts_clear(s, "a")
        run.run()
        st = sk.stats()
        got = [K.decrypt_char(run.result_char(ch)) for ch in outs]
        want = [py_find(buf, p.encode(), **kw) for p, kw in cases]
        assert want == [2, 3, 0, 2, ABSENT, 0] and got == want, (got, want)
        got = [K.decrypt_char(run.result_char(ch)) for ch in flags]
        assert got == py_starts(buf, b"a") == [0, 1, 0, 1, 0, 0], got
        assert 0 < st["max_input_sum_c2"] <= BUDGET
    finally:
        run.close()


# ---- 7. the edges of the C ABI ----------------------------------------------------------------------------------------
NAMES = ("fhs_str_regex_find_clear", "fhs_str_regex_find_clear_wide", "fhs_str_regex_starts_clear")


def test_names_prototypes_and_the_rust_binding(planner):
    from fhestring_amd import cabi
    funcs = {f[0]: f for f in cabi.parse_header()["funcs"]}
    assert all(name in funcs for name in NAMES)
    L = planner.ctx._L
    head = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p]
    for name, argtypes in zip(NAMES, (head, head + [C.c_void_p], head)):
        f = getattr(L, name)
        assert f.restype is C.c_int and f.argtypes == argtypes, name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(ROOT, "bindings", "fhestring_hip.rs")).read()
    assert all("fn %s(" % name in text for name in NAMES)


def test_argument_errors_record_nothing(planner):
    from fhestring_amd import FhsError, lib
    from fhestring_amd.api import _harr
    sk = planner
    L, h = sk.ctx._L, sk.ctx._h
    s = sk.dummy_string(5)
    long = sk.dummy_string(257)
    gone = sk.dummy_string(1)[0]
    released = gone.h
    del gone
    noisy = sk.find(s, sk.dummy_string(2))                   # its digits would be refreshed if it were loaded
    sk.flush()
    st0, luts0 = sk.stats(), lib().fhs_user_lut_count()
    arr, out, hi = _harr(s.chars[:4] + [noisy]), (C.c_uint64 * 5)(), (C.c_uint64 * 1)()
    bad_s = (C.c_uint64 * 5)(*[c.h for c in s.chars[:4]], released)
    calls = {"find": lambda *a: L.fhs_str_regex_find_clear(h, *a, out), "starts": lambda *a: L.fhs_str_regex_starts_clear(h, *a, out),
             "wide": lambda *a: L.fhs_str_regex_find_clear_wide(h, *a, out, hi)}
    for name, call in calls.items():
        for what, args in (("FHS_REGEX_SEARCH", (arr, 5, b"ab", 2, SEARCH_BIT)), ("search beside ignore_case", (arr, 5, b"ab", 2, 3)),
                           ("an unknown bit", (arr, 5, b"ab", 2, 4)), ("unknown bits", (arr, 5, b"ab", 2, 0x80000001)),
                           ("a released handle", (bad_s, 5, b"ab", 2, 0)), ("a NUL in the pattern", (arr, 5, b"a\0b", 3, 0)),
                           ("a null pattern of length 2", (arr, 5, None, 2, 0)), ("a null string of length 5", (None, 5, b"ab", 2, 0)),
                           ("syntax", (arr, 5, b"a(b", 3, 0))):
            assert call(*args) == ERR_ARG, (name, what)
        assert call(arr, 5, b"a{65}", 5, 0) == ERR_LIMIT, name
    assert L.fhs_str_regex_find_clear(h, arr, 5, b"ab", 2, 0, None) == ERR_ARG
    assert L.fhs_str_regex_starts_clear(h, arr, 5, b"ab", 2, 0, None) == ERR_ARG
    assert L.fhs_str_regex_find_clear_wide(h, arr, 5, b"ab", 2, 0, None, hi) == ERR_ARG
    assert L.fhs_str_regex_find_clear_wide(h, arr, 5, b"ab", 2, 0, out, None) == ERR_ARG
    assert L.fhs_str_regex_find_clear(None, arr, 5, b"ab", 2, 0, out) == ERR_ARG
    for mode in (0, 1):                                      # the narrow form's limit, nullable patterns included
        sk.set_mode(mode)
        for pattern in ("ab", "a*"):
            with pytest.raises(FhsError) as err:
                sk.regex_find_clear(long, pattern)
            assert err.value.code == ERR_LIMIT
        with pytest.raises(FhsError) as err:
            sk.regex_find_clear(s, "a(b")
        assert err.value.code == ERR_ARG and "unbalanced" in str(err.value)
    sk.set_mode(1)
    sk.flush()
    assert sk.stats() == st0 and lib().fhs_user_lut_count() == luts0     # no node, no bootstrap, no block, no table
    wide = sk.regex_find_clear_wide(long, "ab")              # the wide form takes 257 characters
    assert wide.trivial_value() is None
    a, wa, _ = _flush_stats(sk, lambda: sk.regex_find_clear(s, b"a.*", ignore_case=True))      # bytes and str alike
    b, wb, _ = _flush_stats(sk, lambda: sk.regex_find_clear(s, "a.*", ignore_case=True))
    assert (a["pbs_executed"], a["pbs_extracted"], wa) == (b["pbs_executed"], b["pbs_extracted"], wb) and a["pbs_executed"] > 0
