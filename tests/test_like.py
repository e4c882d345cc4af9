"""like_clear: SQL LIKE / ILIKE against a clear pattern.  The reference has no such method; the
semantics are stated here in Python, on the buffer's bytes as they are:

    re.match(rb'\\A' + body + rb'(?=\\x00|\\Z)', buf, re.S | (re.I if ignore_case else 0))

with body = [\\x00-\\xff]* for `%`, [^\\x00] for `_` and the escaped byte for a literal.  All on the CPU:

* the logic by constant folding on a planner context, fused and as written, against the regular expression and against
  each other: a fixed list of pattern shapes on buffers of seven sizes, and a seeded random sweep;
* the bookkeeping on uploaded inputs: '%lit%' records what contains_clear(lit) records, the width of the first level,
  the noise budget, the result's noise, linear growth, and the pinned figures of tests/golden/like_plan.json
  (tools/gen_like_plan.py);
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

import gen_like_plan as gen  # noqa: E402

BUDGET = 64
ERR_ARG = -1
TEXT = b"the quick brown foxes jump over the lazy dog; then it ends here."
assert len(TEXT) == 64


# ---- the semantics, in Python ---------------------------------------------------------------------------------------
def tokens(pattern, escape=None):
    """[('lit', byte) | ('one',) | ('any',)] of a pattern (bytes)"""
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i:i + 1]
        if escape is not None and c == escape:
            i += 1
            out.append(("lit", pattern[i:i + 1]))
        elif c == b"%":
            out.append(("any",))
        elif c == b"_":
            out.append(("one",))
        else:
            out.append(("lit", c))
        i += 1
    return out


def py_like(buf, pattern, escape=None, ignore_case=False):
    body = b"".join({"any": rb"[\x00-\xff]*", "one": rb"[^\x00]"}.get(t[0]) or re.escape(t[1]) for t in tokens(pattern, escape))
    return int(re.match(rb"\A" + body + rb"(?=\x00|\Z)", bytes(buf), re.S | (re.I if ignore_case else 0)) is not None)


def test_the_python_statement_itself():
    """what the regular expression says on the cases the design argues with"""
    buf = b"abc\0\0"
    assert [py_like(buf, p) for p in (b"abc", b"ab", b"abc_", b"abc%", b"%", b"", b"a%c", b"_b_", b"%\0%")] == \
        [1, 0, 0, 1, 1, 0, 1, 1, 1]
    assert py_like(b"\0\0", b"") == 1 and py_like(b"", b"") == 1 and py_like(b"", b"%") == 1 and py_like(b"", b"_") == 0
    assert py_like(b"a\0b\0", b"a%b") == 1 and py_like(b"a\0b\0", b"a_b") == 0          # % runs across a NUL, _ does not
    assert py_like(b"a%b", b"a\\%b", escape=b"\\") == 1 and py_like(b"axb", b"a\\%b", escape=b"\\") == 0
    assert py_like(b"aBc", b"AbC") == 0 and py_like(b"aBc", b"AbC", ignore_case=True) == 1
    assert py_like(b"[", b"{", ignore_case=True) == 0                                   # 0x5B / 0x7B: not letters


# ---- fixtures -------------------------------------------------------------------------------------------------------
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


def _both_modes(sk, s, buf, pattern, escape=None, ignore_case=False):
    """like_clear in both modes on a trivially encrypted string: the common value, checked against Python"""
    want = py_like(buf, pattern, escape, ignore_case)
    got = []
    for mode in (1, 0):
        sk.set_mode(mode)
        got.append(sk.like_clear(s, pattern, escape=escape, ignore_case=ignore_case).trivial_value())
    assert got == [want, want], (bytes(buf), pattern, escape, ignore_case, got, want)
    return want


# ---- 1. folding against the regular expression ----------------------------------------------------------------------
MANY = b"%" + b"%".join(TEXT[i:i + 1] for i in range(0, 48, 3)) + b"%"        # 16 one-character segments
FIXED = [b"the%", b"%foxes", b"%fox", b"%quick%brown%", b"%brown%quick%", b"the quick brown foxes",
         b"the quick brown foxe_", b"the quick brown foxes_", b"t__ %", b"%", b"", b"THE Q%FOXES", b"%%", b"t%%e", b"%%e%%",
         b"_%_", b"_", b"%_", b"_%", b"__", b"t%", b"%t", b"T", b"t_e%",
         b"the quick brown f%",                               # a segment of 17 characters: two levels of the AND
         b"%he quick brown foxes jump%", b"%e quick brown fox__ jump over%here.", b"the quick brown foxes jump over the l%_",
         MANY, MANY[1:], MANY[:-1], b"%;%"]
assert len(tokens(MANY)) == 33 and sum(t[0] != "any" for t in tokens(MANY)) == 16


def _buffers(n):
    """canonical buffers (text, then NUL padding) and buffers with NULs inside"""
    out = [TEXT[:n], TEXT[:max(0, n - 3)] + bytes(min(n, 3)), bytes(n)]
    out.append(bytes(0 if i % 7 == 3 else c for i, c in enumerate(TEXT[:n])))
    out.append(bytes(0 if i % 5 == 1 else c for i, c in enumerate(TEXT[:max(0, n - 1)])) + bytes(min(n, 1)))
    if n >= 24:
        out.append(b"the quick brown foxes" + bytes(n - 21))
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 5, 16, 17, 64])
def test_fixed_patterns_fold_to_the_regex(folded, n):
    sk = folded
    hits = 0
    for buf in _buffers(n):
        assert len(buf) == n
        s = _triv(sk, buf)
        text = buf.rstrip(b"\0")
        own = [TEXT[:n + 1], b"_" * (n + 1), b"%" + b"_" * (n + 1), b"_" * n, b"_" * n + b"%"]   # longer than the buffer, and as long
        if text and b"\0" not in text:
            own += [text, text[:-1] + b"_", text + b"%", b"%" + text[-3:], text[:1] + b"%" + text[-1:], text.upper()]
        for pattern in FIXED + own:
            for ignore_case in (False, True):
                hits += _both_modes(sk, s, buf, pattern, ignore_case=ignore_case)
    assert hits >= 10
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0         # everything folded


def test_escapes_fold_to_the_regex(folded):
    sk = folded
    for buf in (b"50% off\0", b"50_ off\0", b"50\\ off\0", b"50x off\0", b"a_b%c\\\0\0"):
        s = _triv(sk, buf)
        for pattern, esc in ((b"50\\% o%", b"\\"), (b"50\\_%", b"\\"), (b"50\\\\%", b"\\"), (b"50!% off", b"!"), (b"50_ off", None),
                             (b"5\\%%", b"\\"), (b"a\\_b\\%c\\\\", b"\\"), (b"a_bx%cxx%", b"x"), (b"%\\%%", b"\\"), (b"%!_%", b"!")):
            for ignore_case in (False, True):
                _both_modes(sk, s, buf, pattern, esc, ignore_case)
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0


def _random_case(rng):
    """(buffer, pattern) over abAB + NUL: up to 9 bytes, 40 % with NULs inside, the others text then padding; up to 6 tokens,
    half of the patterns drawn from the buffer itself (runs replaced by %, characters by _ or the other case)"""
    n = rng.randint(0, 9)
    if rng.random() < 0.4:
        buf = bytes(rng.choice(b"abAB\0\0") for _ in range(n))
    else:
        k = rng.randint(0, n)
        buf = bytes(rng.choice(b"abAB") for _ in range(k)) + bytes(n - k)
    m = rng.randint(0, 6)
    if rng.random() < 0.5:
        toks, i = [], 0
        text = buf.rstrip(b"\0")
        while i < len(text) and len(toks) < m:
            r = rng.random()
            if r < 0.3:
                toks.append(b"%")
                i += rng.randint(0, 3)
            elif r < 0.45 and text[i]:
                toks.append(b"_")
                i += 1
            elif text[i]:
                toks.append(bytes([text[i] ^ 0x20]) if r > 0.9 else text[i:i + 1])
                i += 1
            else:
                toks.append(b"%")
                i += 1
        if i < len(text) and toks and rng.random() < 0.8:
            toks[-1] = b"%"
        pattern = b"".join(toks)
    else:
        pattern = bytes(rng.choice(b"abAB%%_") for _ in range(m))
    return buf, pattern


def test_random_sweep_folds_to_the_regex(folded):
    sk = folded
    rng = random.Random(20)
    total = hits = with_nuls = 0
    for _ in range(1100):
        buf, pattern = _random_case(rng)
        s = _triv(sk, buf)
        with_nuls += b"\0" in buf.rstrip(b"\0")
        for ignore_case in (False, True):
            hits += _both_modes(sk, s, buf, pattern, ignore_case=ignore_case)
            total += 1
    assert total >= 2000 and hits >= 0.10 * total, (total, hits)      # judged by the regular expression alone
    assert hits <= 0.6 * total and with_nuls >= 100, (total, hits, with_nuls)
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0


# ---- 2. bookkeeping on uploaded inputs (fused) ----------------------------------------------------------------------
def _flush_stats(sk, fn):
    sk.flush()
    sk.stats(reset=True)
    keep = fn()
    sk.flush()
    return sk.stats(), sk.level_widths(), keep


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("lit", ["ma", "brown"])
def test_infix_pattern_records_what_contains_clear_records(planner, n, lit):
    """the parity anchor: '%lit%' is contains_clear(lit), node for node"""
    sk = planner
    s = sk.dummy_string(n)
    a, wa, _ = _flush_stats(sk, lambda: sk.contains_clear(s, lit))
    b, wb, _ = _flush_stats(sk, lambda: sk.like_clear(s, "%" + lit + "%"))
    assert a["pbs_executed"] > 0 and wa == wb
    for k in ("pbs_executed", "pbs_extracted", "levels", "max_level_width", "max_input_sum_c2"):
        assert a[k] == b[k], (k, a[k], b[k])
    c, wc, _ = _flush_stats(sk, lambda: sk.like_clear(s, "%%" + lit + "%%%"))       # adjacent % are one
    assert (c["pbs_executed"], c["pbs_extracted"], wc) == (a["pbs_executed"], a["pbs_extracted"], wa)


@pytest.mark.parametrize("n", [64, 17])
def test_first_level_budget_and_result_noise(planner, n):
    """Level 1 holds the rotations of the characters and nothing else: two nibble rotations and one zero test each, the
    zero tests only if the pattern has a `_` or an end anchor; ignore_case adds extractions, not rotations."""
    sk = planner
    s = sk.dummy_string(n)
    for pattern in FIXED + [b"%error%timeout%", b"INV-2024-%", b"%@example.___"]:
        widths = {}
        for ignore_case in (False, True):
            st, w, res = _flush_stats(sk, lambda: sk.like_clear(s, pattern, ignore_case=ignore_case))
            fixed = sum(t[0] != "any" for t in tokens(pattern))
            if fixed > n or (fixed == 0 and pattern):
                assert st["pbs_executed"] == 0 and res.trivial_value() == int(fixed == 0), pattern
                continue
            assert res.trivial_value() is None and res.sum_c2() <= 4, (pattern, res.sum_c2())
            assert 0 < st["max_input_sum_c2"] <= BUDGET, (pattern, ignore_case, st)
            assert st["levels"] == len(w) and w[0] <= 3 * n, (pattern, w)
            if b"_" not in pattern and pattern.endswith(b"%"):
                assert w[0] <= 2 * n, (pattern, w)
            widths[ignore_case] = w
            del res                                          # (a live result would be found again: common subexpressions)
        if widths:
            assert widths[True][0] == widths[False][0], (pattern, widths)             # no rotation added to level 1
            assert len(widths[True]) == len(widths[False])


def test_ignore_case_sums_two_extractions_of_one_rotation(planner):
    sk = planner
    s = sk.dummy_string(64)
    a, wa, _ = _flush_stats(sk, lambda: sk.like_clear(s, "%error%"))
    b, wb, _ = _flush_stats(sk, lambda: sk.like_clear(s, "%error%", ignore_case=True))
    assert wa == wb and a["pbs_executed"] == b["pbs_executed"]
    assert b["pbs_extracted"] > a["pbs_extracted"]                                     # the other case's rows ride along
    assert a["max_input_sum_c2"] < b["max_input_sum_c2"] <= 8 * 4 + 7                   # 15 flags, at most 8 of them sums of two
    c, wc, _ = _flush_stats(sk, lambda: sk.like_clear(s, "%2024-%", ignore_case=True))  # no letter: nothing changes
    d, wd, _ = _flush_stats(sk, lambda: sk.like_clear(s, "%2024-%"))
    assert (c, wc) == (d, wd)


@pytest.mark.parametrize("pattern,ignore_case", [("%ma%", False), ("the%", False), ("%foxes", False), ("a%b%c", False),
                                                 ("%ab%cd%", True), ("t__ %", False), ("%a%b%", False),
                                                 ("%error%timeout%", True), ("%@example.___", False),
                                                 ("a%b%c%d%e%f", False)])
def test_cost_grows_linearly(pattern, ignore_case):
    """Executed bootstraps at 256 against 64 characters: at most 4.2 times as many -- 4, and the rounding of the trees.
    A pattern of T tokens other than % has n - T + 1 windows per segment, and 193 / 53 = 4.62 for T = 12 is linear growth
    all the same: the windows alone allow (257 - T) / (65 - T) <= 4.2 up to T = 5, so the bound is asserted up to there,
    and for every pattern the two equal steps 64 -> 160 -> 256 must cost the same (a quadratic term would make the
    second 1.86 times the first; 5 % for the trees' rounding)."""
    cost = {n: gen.measure_like(pattern, ignore_case, n) for n in (64, 160, 256)}
    pbs = {n: cost[n]["pbs_executed"] for n in cost}
    assert pbs[64] > 0
    if sum(ch != "%" for ch in pattern) <= 5:
        assert pbs[256] <= 4.2 * pbs[64], pbs
    assert pbs[256] - pbs[160] <= 1.05 * (pbs[160] - pbs[64]), pbs
    assert max(cost[n]["max_input_sum_c2"] for n in cost) <= BUDGET


def test_noisy_operands_stay_within_the_budget(planner):
    """characters that are sums of bootstrap outputs (a case fold, a select) are refreshed where the nibble packing would
    leave the budget, as everywhere else"""
    sk = planner
    s = sk.dummy_string(17)
    noisy = sk.to_upper(s)
    cut = sk.take(s, sk.dummy_string(1)[0])
    sk.flush()
    for operand in (noisy, cut):
        for pattern, ic in (("%AB_", False), ("a%b%c", True), ("", False), ("_%", False)):
            st, _, res = _flush_stats(sk, lambda: sk.like_clear(operand, pattern, ignore_case=ic))
            assert 0 < st["max_input_sum_c2"] <= BUDGET and res.sum_c2() <= 4, (pattern, st, res.sum_c2())
            del res


def test_pinned_plan():
    """The figures of tests/golden/like_plan.json (DESIGN section 20 quotes them): a change there is a change of the DAG."""
    with open(gen.PATH) as f:
        pinned = json.load(f)
    assert len(gen.CASES) == 6 and sorted(pinned["cases"]) == sorted(gen.key(*c) for c in gen.CASES)
    for case in gen.CASES:
        got = gen.measure_like(*case)
        assert got == pinned["cases"][gen.key(*case)], case
        assert got["pbs_executed"] > 0 and got["max_input_sum_c2"] <= BUDGET and got["result_sum_c2"] <= 4


# ---- 3. real ciphertexts, the CPU oracle's bootstrap ----------------------------------------------------------------
def test_results_decrypt_on_real_ciphertexts(oracle_keys, oracle_sk):
    from oracle.plan_exec import PlanRun
    K = oracle_keys
    run = PlanRun(oracle_sk, threads=min(16, os.cpu_count() or 1), mode=6)
    try:
        sk = run.sk
        buf = b"zama!\0"
        s = run.upload_string(np.stack([K.encrypt_char(b) for b in buf]))
        cases = [("za%", False), ("zb%", False),             # a prefix
                 ("%ma_", False), ("%ma", False),            # `_`, and the end anchor
                 ("Z%M%!", True), ("%!%a%", True)]           # two extractions summed; the order of segments
        outs = [sk.like_clear(s, p, ignore_case=ic) for p, ic in cases]
        run.run()
        st = sk.stats()
        got = [K.decrypt_char(run.result_char(ch)) for ch in outs]
        want = [py_like(buf, p.encode(), ignore_case=ic) for p, ic in cases]
        assert want == [1, 0, 1, 0, 1, 0] and got == want, (got, want)
        assert 0 < st["max_input_sum_c2"] <= BUDGET and 20 < run.pbs < 400, run.pbs
    finally:
        run.close()


# ---- 4. the edges of the C ABI ----------------------------------------------------------------------------------------
def test_name_prototype_and_the_rust_binding(planner):
    from fhestring_amd import cabi
    funcs = {f[0]: f for f in cabi.parse_header()["funcs"]}
    assert "fhs_str_like_clear" in funcs and dict(cabi.parse_header()["consts"])["FHS_LIKE_IGNORE_CASE"] == 1
    f = planner.ctx._L.fhs_str_like_clear
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.c_uint32, C.c_void_p]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(ROOT, "bindings", "fhestring_hip.rs")).read()
    assert "fn fhs_str_like_clear(" in text and "FHS_LIKE_IGNORE_CASE" in text


def test_argument_errors_record_nothing(planner):
    from fhestring_amd import FhsError
    from fhestring_amd.api import _harr
    sk = planner
    L, h = sk.ctx._L, sk.ctx._h
    s = sk.dummy_string(5)
    noisy = sk.find(s, sk.dummy_string(2))                   # its digits would be refreshed if it were loaded
    gone = sk.dummy_string(1)[0]
    released = gone.h
    del gone
    sk.flush()
    assert noisy.sum_c2() > 4
    st0 = sk.stats()
    arr, out = _harr(s.chars + [noisy]), (C.c_uint64 * 1)()
    bad_s = (C.c_uint64 * 5)(*[c.h for c in s.chars[:4]], released)
    like = L.fhs_str_like_clear
    bad = [("a NUL in the pattern", lambda: like(h, arr, 6, b"a\0b", 3, -1, 0, out)),
           ("escape 0", lambda: like(h, arr, 6, b"ab", 2, 0, 0, out)),
           ("escape %", lambda: like(h, arr, 6, b"ab", 2, ord("%"), 0, out)),
           ("escape _", lambda: like(h, arr, 6, b"ab", 2, ord("_"), 0, out)),
           ("escape 256", lambda: like(h, arr, 6, b"ab", 2, 256, 0, out)),
           ("escape -2", lambda: like(h, arr, 6, b"ab", 2, -2, 0, out)),
           ("escape at the end", lambda: like(h, arr, 6, b"ab\\", 3, ord("\\"), 0, out)),
           ("escape before a letter", lambda: like(h, arr, 6, b"a\\b", 3, ord("\\"), 0, out)),
           ("escape before a NUL", lambda: like(h, arr, 6, b"a\\\0", 3, ord("\\"), 0, out)),
           ("unknown flag bits", lambda: like(h, arr, 6, b"ab", 2, -1, 2, out)),
           ("unknown flag bits beside the known one", lambda: like(h, arr, 6, b"ab", 2, -1, 0x80000001, out)),
           ("a null out", lambda: like(h, arr, 6, b"ab", 2, -1, 0, None)),
           ("a null pattern of length 2", lambda: like(h, arr, 6, None, 2, -1, 0, out)),
           ("a null context", lambda: like(None, arr, 6, b"ab", 2, -1, 0, out)),
           ("a released handle", lambda: like(h, bad_s, 5, b"ab", 2, -1, 0, out)),
           ("a null string of length 5", lambda: like(h, None, 5, b"ab", 2, -1, 0, out))]
    for name, call in bad:
        assert call() == ERR_ARG, name
    for kw in ({"escape": "%"}, {"escape": b"\0"}):          # ... and through the method: what _check raises for FHS_ERR_ARG
        with pytest.raises(FhsError) as err:
            sk.like_clear(s, "ab", **kw)
        assert err.value.code == ERR_ARG
    with pytest.raises(FhsError):
        sk.like_clear(s, "ab!", escape="!")
    with pytest.raises(ValueError):
        sk.like_clear(s, "ab", escape="!!")
    # decided by the token counts alone: nothing is loaded, the noisy operand is not refreshed
    chars = s.chars + [noisy]
    assert sk.like_clear(chars, "_______").trivial_value() == 0 and sk.like_clear(chars, "%%").trivial_value() == 1
    sk.flush()
    assert sk.stats() == st0                                 # no node, no bootstrap, no block


def test_empty_string_and_pattern_forms(planner):
    from fhestring_amd.api import FheAsciiChar
    sk = planner
    L, h = sk.ctx._L, sk.ctx._h
    st0 = sk.stats()
    for mode in (0, 1):
        sk.set_mode(mode)
        assert sk.like_clear([], "").trivial_value() == 1 and sk.like_clear([], "%").trivial_value() == 1
        assert sk.like_clear([], "_").trivial_value() == 0 and sk.like_clear([], "a%").trivial_value() == 0
        out = (C.c_uint64 * 1)()
        assert L.fhs_str_like_clear(h, None, 0, None, 0, -1, 0, out) == 0           # n == 0 and m == 0 need no pointers
        assert FheAsciiChar(sk, out[0]).trivial_value() == 1
    sk.set_mode(1)
    sk.flush()
    assert sk.stats() == st0
    s = sk.dummy_string(4)
    a, wa, _ = _flush_stats(sk, lambda: sk.like_clear(s, b"a%", escape=b"\\", ignore_case=True))   # bytes for both
    b, wb, _ = _flush_stats(sk, lambda: sk.like_clear(s, "a%", escape="\\", ignore_case=True))
    assert (a["pbs_executed"], a["pbs_extracted"], wa) == (b["pbs_executed"], b["pbs_extracted"], wb) == (3, 1, [2, 1])   # two nibbles, one AND
    e, we, res = _flush_stats(sk, lambda: sk.like_clear(s, ""))                    # the empty pattern: s[0] == 0, one bootstrap
    assert (e["pbs_executed"], we) == (1, [1]) and res.sum_c2() == 1
