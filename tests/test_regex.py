"""regex_clear: regular expressions against a clear pattern.  The reference has no such method; the
semantics are Python's own, on text = the buffer up to its first NUL:

    re.fullmatch(pattern, text, re.S | (re.I if ignore_case else 0))          re.search with search=True

and the accepted syntax is a strict subset of Python's, so `re` is the oracle without any translation.  All on the CPU:

* the parser alone (fhs_regex_info): positions and shortest match of every accepted construct, the offset of every
  refused one, the position limit;
* the logic by constant folding on a planner context, fused and as written, against `re` and against each other: a
  fixed list of patterns on buffers of seven sizes, and a seeded random sweep;
* the bookkeeping on uploaded inputs: the noise budget, the result's noise, the depth bound, pruning, literals without
  tables, and the pinned figures of tests/golden/regex_plan.json (tools/gen_regex_plan.py);
* real ciphertexts through the CPU oracle's bootstrap (oracle/plan_exec.py);
* the edges of the C ABI."""
import ctypes as C
import json
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_regex_plan as gen  # noqa: E402

BUDGET = 64
ERR_ARG, ERR_LIMIT = -1, -4
TEXT = b"AB-2024 error: Quick brown fox hit a timeout at host@site.org !!"
assert len(TEXT) == 64


def py_regex(buf, pattern, ignore_case=False, search=False):
    text = bytes(buf).split(b"\0")[0]
    fn = re.search if search else re.fullmatch
    return int(fn(pattern, text, re.S | (re.I if ignore_case else 0)) is not None)


def info(pattern, **kw):
    from fhestring_amd.api import MyServerKey
    return MyServerKey.regex_info(pattern, **kw)


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


def _both_modes(sk, s, buf, pattern, ignore_case=False, search=False):
    """regex_clear in both modes on a trivially encrypted string: the common value, checked against Python"""
    want = py_regex(buf, pattern, ignore_case, search)
    got = []
    for mode in (1, 0):
        sk.set_mode(mode)
        got.append(sk.regex_clear(s, pattern, ignore_case=ignore_case, search=search).trivial_value())
    assert got == [want, want], (bytes(buf), pattern, ignore_case, search, got, want)
    return want


# ---- 1. the parser --------------------------------------------------------------------------------------------------
ACCEPTED = [                                                  # (pattern, positions, shortest match)
    (b"", 0, 0), (b"abc", 3, 3), (rb"a\.b\\\*\ \-", 7, 7), (rb"\t\n\r\f\v\0\x41\x7f", 8, 8), (b".", 1, 1),
    (rb"\d\w\s\D\W\S", 6, 6), (b"[abc]", 1, 1), (b"[a-z0-9_]", 1, 1), (b"[^a-z]", 1, 1), (rb"[\d\-\]x\x41-\x43]", 1, 1),
    (b"[a-]", 1, 1), (b"[-a]", 1, 1), (b"[^-]", 1, 1), (rb"[\0a]", 1, 1), (b"(ab)", 2, 2), (b"(?:ab)c", 3, 3),
    (b"a|bc", 3, 1), (b"a||b", 2, 0), (b"|", 0, 0), (b"()", 0, 0), (b"(?:)*", 0, 0), (b"a*", 1, 0), (b"a+", 1, 1),
    (b"a?", 1, 0), (b"a{3}", 3, 3), (b"a{2,}", 2, 2), (b"a{0,}", 1, 0), (b"a{2,4}", 4, 2), (b"a{0}", 0, 0),
    (b"(ab|c){2}", 6, 2), (b"(a|bc)*d?", 4, 0), (b"((a|b)(c|d)){2,3}e", 13, 5), (b"a}b]", 4, 4),
    (b"[A-Z]{2}-[0-9]+", 4, 4), (b"(error|warn).*timeout", 17, 11), (rb"\w+@\w+\.(com|org)", 10, 7), (b"a{64}", 64, 64),
    (b"(a{8}){8}", 64, 64), (b"(?:a{0}){1000000}", 0, 0), (b"(){5}", 0, 0),
]
REFUSED = [                                                   # (pattern, offset of what is refused)
    (b"^a", 0), (b"a$", 1), (rb"a\b", 1), (rb"\Ba", 0), (rb"\Aa", 0), (rb"a\Z", 1),                 # anchors
    (rb"(a)\1", 3), (rb"\8", 0), (rb"a\07", 1),                                                    # back-references, octal
    (b"(?=a)", 0), (b"a(?!b)", 1), (b"(?<=a)b", 0), (b"(?<!a)b", 0),                               # look-around
    (b"(?i)a", 0), (b"(?P<n>a)", 0), (b"a(?i:b)", 1), (b"(?#c)a", 0),                              # inline flags, names
    (b"a*?", 2), (b"a+?", 2), (b"a??", 2), (b"a{2}?", 4), (b"a*+", 2), (b"a++", 2), (b"a**", 2), (b"a{2}{3}", 4),
    (b"*a", 0), (b"a|+", 2), (b"(?:?)", 3), (b"{2}", 0),                                           # nothing to repeat
    (b"a{", 1), (b"a{,3}", 1), (b"a{x}", 1), (b"a{2", 1), (b"a{2,x}", 1),                          # not a counted form
    (b"a\0b", 1), (b"[a\0]", 2), (b"\\\0", 1),                                                     # a NUL byte
    (b"(a", 0), (b"a)", 1), (b"((a)", 0), (b"a(b))", 4), (b"[a", 0), (b"a[b-", 1), (b"a[^", 1),     # unbalanced
    (b"[]", 0), (b"a[^]", 1), (b"[]a]", 0),                                                        # an empty class
    (b"[z-a]", 1), (rb"[\x42-\x41]", 1), (b"a{3,2}", 1), (b"[a-\\d]", 1), (b"[\\d-z]", 1),          # reversed, shorthand ends
    (b"[[a]", 1), (b"[a--b]", 1), (b"[--a]", 1), (b"[a&&b]", 2), (rb"[\b]", 1), (rb"\e", 0), (rb"\x4", 0), (rb"\xg1", 0), (b"a\\", 1),
]


def test_accepted_constructs():
    for pattern, positions, low in ACCEPTED:
        re.compile(pattern)                                   # a subset of Python's syntax
        assert info(pattern) == {"code": 0, "positions": positions, "min_len": low}, pattern
        assert info(pattern, ignore_case=True) == {"code": 0, "positions": positions, "min_len": low}, pattern
        if positions <= 62:                                   # search: .*(?:pattern).*, two more positions
            assert info(pattern, search=True) == {"code": 0, "positions": positions + 2, "min_len": low}, pattern


def test_refused_constructs_and_their_offsets():
    for pattern, offset in REFUSED:
        for kw in ({}, {"ignore_case": True, "search": True}):
            assert info(pattern, **kw) == {"code": ERR_ARG, "err_offset": offset}, pattern


def test_the_position_limit():
    assert info(b"a{64}")["code"] == 0 and info(b"a{64}", search=True)["code"] == ERR_LIMIT
    for pattern in (b"a{65}", b"(a{5}){13}", b"(ab|c){22}", b"a{1000000000000}", b"a{70,}", b"a{0,65}", b"a" * 65,
                    b"(" * 65 + b"a" + b")" * 65, b"a?" * 1025,
                    # trees that would be deep without a single position: empty branches and empty groups
                    b"|" * 1025, b"|" * 100000, b"a|" * 600, b"()" * 1025, b"(?:)|" * 40000, b"(|)" * 600, b"a" * 200000):
        assert info(pattern) == {"code": ERR_LIMIT, "err_offset": 0}, pattern[:40]
        assert info(pattern, ignore_case=True, search=True) == {"code": ERR_LIMIT, "err_offset": 0}, pattern[:40]
    assert info(b"|" * 1024) == {"code": 0, "positions": 0, "min_len": 0}             # 1024 '|': the most that is taken
    assert info(b"()" * 1024) == {"code": 0, "positions": 0, "min_len": 0}
    assert info(b"|".join([b"a"] * 32) * 2)["code"] == 0
    from fhestring_amd import lib
    f = lib().fhs_regex_info                                  # null pointers, a null pattern, unknown flag bits
    assert f(b"ab", 2, 0, None, None, None) == 0 and f(b"a{65}", 5, 0, None, None, None) == ERR_LIMIT
    assert f(None, 0, 0, None, None, None) == 0 and f(None, 2, 0, None, None, None) == ERR_ARG
    assert f(b"ab", 2, 4, None, None, None) == ERR_ARG and f(b"ab", 2, 0x80000001, None, None, None) == ERR_ARG


def test_refused_patterns_record_nothing(planner):
    from fhestring_amd import FhsError, lib
    sk = planner
    s = sk.dummy_string(5)
    noisy = sk.find(s, sk.dummy_string(2))                   # its digits would be refreshed if it were loaded
    sk.flush()
    st0, luts0 = sk.stats(), lib().fhs_user_lut_count()
    over = (b"a{65}", b"[a-c]{65}", b"|" * 100000, b"()" * 1025)
    for pattern, code in [(p, ERR_ARG) for p, _ in REFUSED] + [(p, ERR_LIMIT) for p in over]:
        for mode in (0, 1):
            sk.set_mode(mode)
            with pytest.raises(FhsError) as err:
                sk.regex_clear(s.chars + [noisy], pattern)
            assert err.value.code == code, pattern[:40]
    sk.set_mode(1)
    sk.flush()
    assert sk.stats() == st0 and lib().fhs_user_lut_count() == luts0


# ---- 2. folding against Python ----------------------------------------------------------------------------------------
FIXED = [
    # every quantifier
    b"AB-2024.*", b"A?AB-[0-9]+ .*", b"[A-Z]{2}-[0-9]{4} .*", b"[A-Z]{2,}-\\d{2,5}.*", b".{3}.*", b".{0,3}", b".{2}", b"A+B?-?.*",
    b"a{2}", b"x*", b"A*", b".+", b".?", b"[A-Z]+",
    # nested groups, alternation with branches of unequal length
    b"((A|a)(B|b))-((20|19)(24)) .*", b"(?:(?:AB)-)+.*", b"(AB-2024|A|AB).*", b"(A|AB|AB-)(B|-|2)[0-9-]*( .*)?", b"(a|ab)(c|bcd)(d*)",
    b"(AB|A)(B-|-)?2.*", b"(error|warn).*timeout", b"AB-(2024|20) (error|warn)(: | ).*",
    # nullable patterns
    b"", b"(ab|cd)*e?", b"a*", b"(A|B)*", b"(AB)?(-2024)?",
    # a position with more than six predecessors
    b"[A-Z](a|b|c|d|e|f|g|h|B)[-x].*", b"(A|B|-|2|0|4| |e)+.*",
    # negated classes and ranges
    b"[^a]B-.*", b"[^A]B-.*", b"[Z-a]+", b"[^Z-a]+.*", b"[^0-9]{3}[^a-z]{4}.*", rb"\w\w\W\d+\s\S+.*", rb"\D+\d+\D+",
    # classes with escapes, literal escapes
    rb"AB\-2024\ error\:.*", rb"[\x41][\x42-\x43]-.*", rb"[\w-]+ [a-z:]+.*", rb".*\.org !!", rb".*@[a-z]+\.(com|org).*",
    rb".*\0.*", rb"A\x00?B.*", rb"[\0A]B.*",
    b"A", b"AB", b".*", b".*!", b".*[^!]",
]
SEARCHES = [b"AB-", b"ab-2", b"brown", b"BROWN", b"!!", b"org !!", b"timeout", b"(error|warn).*timeout", b"fox|dog", b"xyz",
            b"[0-9]{4}", b"[0-9]{5}", b"q[a-z]+k", b"", b"x*", b"@[a-z]+\\.", b"t a t", b"[^ -~]"]


def _buffers(n):
    """canonical buffers (text, then NUL padding) and buffers with NULs inside"""
    out = [TEXT[:n], TEXT[:max(0, n - 3)] + bytes(min(n, 3)), bytes(n)]
    out.append(bytes(0 if i % 7 == 3 else c for i, c in enumerate(TEXT[:n])))
    out.append(bytes(0 if i == 9 else c for i, c in enumerate(TEXT[:max(0, n - 1)])) + bytes(min(n, 1)))
    if n >= 8:
        out.append(b"Za_zA`" + bytes(n - 6))
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 5, 16, 17, 64])
def test_fixed_patterns_fold_to_python(folded, n):
    sk = folded
    hits = total = 0
    for buf in _buffers(n):
        assert len(buf) == n
        s = _triv(sk, buf)
        text = buf.split(b"\0")[0][:20]
        own = [b"." * min(n + 1, 64), b"." * n, b".{%d}" % min(n, 60), b"[^x]{%d,}" % min(n, 60)]
        if text:
            own += [re.escape(text), re.escape(text[:-1]) + b".", re.escape(text) + b".*", re.escape(text) + b".+",
                    re.escape(text.swapcase())]
        for pattern in FIXED + own:
            for ignore_case in (False, True):
                hits += _both_modes(sk, s, buf, pattern, ignore_case=ignore_case)
                total += 1
        for pattern in SEARCHES + ([re.escape(text[-3:])] if text else []):
            for ignore_case in (False, True):
                hits += _both_modes(sk, s, buf, pattern, ignore_case=ignore_case, search=True)
                total += 1
    assert 0.1 * total <= hits <= 0.9 * total, (hits, total)
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0         # everything folded


def test_search_positions_and_the_first_nul(folded):
    """a match at the start, in the middle, at the end, and only beyond the first NUL"""
    sk = folded
    buf = b"start middle end\0beyond\0"
    s = _triv(sk, buf)
    got = [_both_modes(sk, s, buf, p, search=True) for p in (b"start", b"mid+le", b"end", b"beyond", rb"d\0b", b"e[a-z]d", b"e[a-z]{2}d")]
    assert got == [1, 1, 1, 0, 0, 1, 0]
    assert _both_modes(sk, s, buf, b"start middle end") == 1 and _both_modes(sk, s, buf, b"start.*beyond") == 0
    assert _both_modes(sk, s, buf, b"START.*END", ignore_case=True) == 1 and _both_modes(sk, s, buf, b"START.*END") == 0


def test_ignore_case_means_what_re_I_means(folded):
    sk = folded
    for buf in (b"a", b"A", b"Z", b"z", b"[", b"{", b"`", b"@", b"_", b"k", b"K"):
        s = _triv(sk, buf)
        for pattern in (b"[^a]", b"[Z-a]", b"[^Z-a]", b"[a-z]", b"[^A-Z]", b"[X-c]", b"a", b"A", b"\\W", b"[\\Wk]", b"[^\\Wk]", b"[@-[]",
                        b"[`-{]", b"\\x41", b"[\\x5a-\\x61]"):
            for ignore_case in (False, True):
                _both_modes(sk, s, buf, pattern, ignore_case=ignore_case)


def _random_pattern(rng, depth, text):
    """a pattern over abAB; `text` (maybe empty) steers the literals so that matches are not rare"""
    def atom():
        r = rng.random()
        if text and r < 0.55:
            c = text[rng.randrange(len(text))]
            return bytes([c ^ 0x20 if rng.random() < 0.15 else c])
        return rng.choice([b"a", b"b", b"A", b"B", b".", b"[ab]", b"[^a]", b"[a-b]", b"[A-b]", b"[^B]", b"[aB]", rb"\w", rb"[^\W]"])
    if depth == 0:
        return atom()
    r = rng.random()
    if r < 0.35:
        return b"".join(_random_pattern(rng, depth - 1, text) for _ in range(rng.randint(1, 3)))
    if r < 0.5:
        return b"(" + b"|".join(_random_pattern(rng, depth - 1, text) for _ in range(rng.randint(2, 3))) + b")"
    if r < 0.85:
        inner = _random_pattern(rng, depth - 1, text)
        if len(inner) > 1 and not (inner.startswith(b"[") and inner.endswith(b"]") and inner.count(b"[") == 1) and inner not in (rb"\w",):
            inner = rng.choice([b"(", b"(?:"]) + inner + b")"
        q = rng.choice([b"*", b"+", b"?", b"{2}", b"{1,}", b"{0,2}", b"{1,3}", b"*", b"?"])
        return inner + q
    return _random_pattern(rng, depth - 1, text)


def _random_case(rng):
    n = rng.randint(0, 8)
    if rng.random() < 0.35:
        buf = bytes(rng.choice(b"abAB\0\0") for _ in range(n))
    else:
        k = rng.randint(0, n)
        buf = bytes(rng.choice(b"abAB") for _ in range(k)) + bytes(n - k)
    text = buf.split(b"\0")[0]
    if rng.random() < 0.5 and text:                          # the text itself, loosened here and there
        parts = []
        for c in text:
            r = rng.random()
            parts.append(bytes([c]) if r < 0.5 else rng.choice([b".", b"[abAB]", b"[a-b]?", b"(a|b|A|B)", bytes([c]) + b"+",
                                                                bytes([c]) + b"*", b".*", bytes([c ^ 0x20]), b"[^b]", b"(?:%c|B)" % c]))
        pattern = b"".join(parts)
    else:
        pattern = _random_pattern(rng, rng.randint(1, 3), text)
    return buf, pattern, rng.random() < 0.5, rng.random() < 0.4


def test_random_sweep_folds_to_python(folded):
    sk = folded
    rng = random.Random(22)
    total = hits = with_nuls = 0
    for _ in range(2400):
        buf, pattern, ignore_case, search = _random_case(rng)
        assert info(pattern, search=search)["code"] == 0, pattern     # the generator stays inside the syntax and the limit
        s = _triv(sk, buf)
        with_nuls += b"\0" in buf.rstrip(b"\0")
        hits += _both_modes(sk, s, buf, pattern, ignore_case, search)
        total += 1
    assert total >= 2000 and 0.30 * total <= hits <= 0.70 * total, (total, hits)      # judged by `re` alone
    assert with_nuls >= 100, with_nuls
    sk.set_mode(1)
    assert sk.stats(reset=True)["pbs_executed"] == 0


def test_search_of_a_literal_agrees_with_contains_clear(folded):
    sk = folded
    rng = random.Random(7)
    hits = 0
    for _ in range(300):
        n = rng.randint(1, 12)
        k = rng.randint(0, n)
        buf = bytes(rng.choice(b"abc") for _ in range(k)) + bytes(n - k)
        lit = "".join(rng.choice("abc") for _ in range(rng.randint(1, 3)))
        s = _triv(sk, buf)
        sk.set_mode(1)
        a = sk.contains_clear(s, lit).trivial_value()
        b = sk.regex_clear(s, lit, search=True).trivial_value()
        assert a == b == int(lit.encode() in buf), (buf, lit, a, b)
        hits += a
    assert 60 <= hits <= 240, hits


# ---- 3. bookkeeping on uploaded inputs (fused) ------------------------------------------------------------------------
def _flush_stats(sk, fn):
    sk.flush()
    sk.stats(reset=True)
    keep = fn()
    sk.flush()
    return sk.stats(), sk.level_widths(), keep


def _depth_bound(n):
    return 2 + n + 1 + math.ceil(math.log(n + 1, 15))


# Eight one-byte branches under `+`: 2 * 2 + 8 = 20 does not fit the message space, so at EVERY index the predecessors go
# through or_tree first -- one more level per index, as DESIGN section 22 says.
OR_AT_EVERY_INDEX = (b"(A|B|-|2|0|4| |e)+.*",)


@pytest.mark.parametrize("n", [17, 64])
def test_budget_result_noise_and_depth(planner, n):
    sk = planner
    s = sk.dummy_string(n)
    recorded = 0
    for pattern, search in [(p, False) for p in FIXED] + [(p, True) for p in SEARCHES]:
        for ignore_case in (False, True):
            st, w, res = _flush_stats(sk, lambda: sk.regex_clear(s, pattern, ignore_case=ignore_case, search=search))
            known = res.trivial_value()
            if known is not None:                            # decided by the pattern alone (or a dead position)
                assert st["pbs_executed"] == 0, pattern
                continue
            recorded += 1
            assert 0 < st["max_input_sum_c2"] <= BUDGET, (pattern, ignore_case, st)
            assert res.sum_c2() == 1, (pattern, res.sum_c2())
            assert st["levels"] == len(w)
            assert st["levels"] <= _depth_bound(n) + (n if pattern in OR_AT_EVERY_INDEX else 0), (pattern, st["levels"])
            if pattern in OR_AT_EVERY_INDEX:
                assert st["levels"] > _depth_bound(n)        # the or_tree path was taken
            del res                                          # (a live result would be found again: common subexpressions)
    assert recorded >= 100


def test_trivial_decisions_load_nothing(planner):
    sk = planner
    s = sk.dummy_string(5)
    noisy = sk.find(s, sk.dummy_string(2))
    sk.flush()
    assert noisy.sum_c2() > 4
    st0 = sk.stats()
    chars = s.chars + [noisy]
    for mode in (0, 1):
        sk.set_mode(mode)
        assert sk.regex_clear(chars, ".{7}").trivial_value() == 0 and sk.regex_clear(chars, "abcdefg", search=True).trivial_value() == 0
        assert sk.regex_clear(chars, ".*").trivial_value() == 1 and sk.regex_clear(chars, "(.|a)*").trivial_value() == 1
        assert sk.regex_clear(chars, "a*", search=True).trivial_value() == 1 and sk.regex_clear(chars, "", search=True).trivial_value() == 1
        assert sk.regex_clear([], "a*").trivial_value() == 1 and sk.regex_clear([], "(a|)b?").trivial_value() == 1
        assert sk.regex_clear([], "a").trivial_value() == 0 and sk.regex_clear([], "", search=True).trivial_value() == 1
    sk.set_mode(1)
    sk.flush()
    assert sk.stats() == st0                                 # no node, no bootstrap, no refresh of the noisy operand


def test_noisy_operands_are_refreshed_within_the_budget(planner):
    """characters that are sums of bootstrap outputs (a case fold, a select) are refreshed where the nibble packing would
    leave the budget, as block_eq_flags does it"""
    sk = planner
    s = sk.dummy_string(9)
    noisy = sk.to_upper(s)
    cut = sk.take(s, sk.dummy_string(1)[0])
    sk.flush()
    for operand in (noisy, cut):
        for pattern, kw in (("AB.*", {}), ("[A-Z]+[0-9]?", {}), ("(a|bc)*d", {"ignore_case": True}), ("b[^c]", {"search": True}), ("", {})):
            st, _, res = _flush_stats(sk, lambda: sk.regex_clear(operand, pattern, **kw))
            assert 0 < st["max_input_sum_c2"] <= BUDGET and res.sum_c2() == 1, (pattern, st, res.sum_c2())
            del res


@pytest.mark.parametrize("pattern", ["abc", "error: timeout", "a", r"\.\*x"])
def test_a_literal_pattern_needs_no_table_and_is_pruned(planner, pattern):
    from fhestring_amd import lib
    sk = planner
    length = info(pattern)["positions"]
    luts0 = lib().fhs_user_lut_count()
    cost = {}
    for n in (length + 1, length + 2, 16, 64):
        s = sk.dummy_string(n)
        st, w, res = _flush_stats(sk, lambda: sk.regex_clear(s, pattern))
        assert w[0] <= 2 * n and w[0] == 2 * length + 1, (n, w)           # two nibble rotations per literal, one zero test
        assert st["levels"] == length + 2
        cost[n] = (st["pbs_executed"], st["pbs_extracted"], w)
        del res, s
        s = sk.dummy_string(n)
        _, w2, res = _flush_stats(sk, lambda: sk.regex_clear(s, pattern, ignore_case=True))
        assert w2[0] == w[0]                                 # the other case rides along as an extraction
        del res, s
    assert len(set(map(repr, cost.values()))) == 1, cost     # does not depend on n
    assert cost[64][0] == 2 * length + length + 2            # the nibble tests, one step per character, nz and the end
    assert lib().fhs_user_lut_count() == luts0


def test_distinct_classes_share_their_tables_and_steps_are_one_bootstrap(planner):
    from fhestring_amd import lib
    sk = planner
    n = 16
    s = sk.dummy_string(n)
    _flush_stats(sk, lambda: sk.class_flags(s, "A-Z"))       # registers the tables of [A-Z]
    luts0 = lib().fhs_user_lut_count()
    a, wa, _ = _flush_stats(sk, lambda: sk.class_flags(s, "A-Z"))
    per_char = a["pbs_executed"] // n
    b, wb, _ = _flush_stats(sk, lambda: sk.regex_clear(s, "[A-Z]+"))
    assert lib().fhs_user_lut_count() == luts0               # interned: the same class, the same tables
    # class flags of every character, then one step per index after the first, one zero test and one gate per inner end
    assert b["pbs_executed"] == per_char * n + (n - 1) + 2 * (n - 1) + 2, (a, b)    # ... and the OR of 16 ends: 15 + 1
    assert wb[0] >= wa[0]                                    # the class tests stand at the front


def test_as_written_registers_no_table(planner):
    """the table plans and the threshold tables belong to the fused mode"""
    from fhestring_amd import lib
    sk = planner
    s = sk.dummy_string(4)
    sk.set_mode(0)
    luts0 = lib().fhs_user_lut_count()
    for pattern in ("[a-z]+", "[q-t7]x", "(a|b|c)[d-f]", r"[^\W_]+"):
        res = sk.regex_clear(s, pattern)
        assert res.trivial_value() is None
        del res
    assert lib().fhs_user_lut_count() == luts0
    sk.set_mode(1)
    res = sk.regex_clear(s, "[q-t7]x")                        # the same class, fused: its tables
    assert lib().fhs_user_lut_count() > luts0
    del res


def test_threshold_tables_are_registered_with_the_plan(planner):
    """Every threshold table a step can ask for is registered before the string is loaded (a full registry then fails with
    nothing recorded): a pattern that is decided only on the string registers the same tables on a string too short to
    build the steps that use them as on a long one."""
    from fhestring_amd import lib
    sk = planner
    count = lib().fhs_user_lut_count
    before = count()
    short = sk.dummy_string(2)
    res = sk.regex_clear(short, "(k|l|m)*[n-p]?")              # [n-p] after three branches: needs index 1 at least
    after_short = count()
    assert after_short > before
    del res
    res = sk.regex_clear(sk.dummy_string(9), "(k|l|m)*[n-p]?")
    assert count() == after_short
    del res


def test_pinned_plan():
    """The figures of tests/golden/regex_plan.json (DESIGN section 22 quotes them): a change there is a change of the DAG."""
    with open(gen.PATH) as f:
        pinned = json.load(f)
    assert len(gen.CASES) == 12 and sorted(pinned["cases"]) == sorted(gen.key(*c) for c in gen.CASES)
    for case in gen.CASES:
        got = gen.measure_regex(*case)
        assert got == pinned["cases"][gen.key(*case)], case
        assert got["pbs_executed"] > 0 and got["max_input_sum_c2"] <= BUDGET and got["result_sum_c2"] == 1
        assert got["levels"] <= _depth_bound(case[2])


# ---- 4. real ciphertexts, the CPU oracle's bootstrap ------------------------------------------------------------------
def test_results_decrypt_on_real_ciphertexts(oracle_keys, oracle_sk):
    from oracle.plan_exec import PlanRun
    K = oracle_keys
    run = PlanRun(oracle_sk, threads=min(16, os.cpu_count() or 1), mode=6)
    try:
        sk = run.sk
        buf = b"zama!\0"
        s = run.upload_string(np.stack([K.encrypt_char(b) for b in buf]))
        cases = [("za[a-z]+!", {}), ("za[a-z]+", {}),                      # a class with a user table; the end anchor
                 ("z(am)*a!", {}), ("(zama|ma)", {}),                      # `*` on a group; an alternation
                 ("M[AB]!", {"search": True, "ignore_case": True}), ("am!", {"search": True}),
                 # five one-byte predecessors: 2 * 6 + 5 leaves the message space, so every step goes through or_tree
                 ("(z|a|m|!|x)+", {}), ("(z|a|m|x|y)+", {}),
                 # three and four predecessors of a class position: the threshold tables [v >= 5] and [v >= 6]
                 ("(z|a|m)+[ -/]", {}), ("(z|a|m|!)+[0-9]?", {}), ("(z|a|m)+[0-9]", {})]
        outs = [sk.regex_clear(s, p, **kw) for p, kw in cases]
        run.run()
        st = sk.stats()
        got = [K.decrypt_char(run.result_char(ch)) for ch in outs]
        want = [py_regex(buf, p.encode(), **kw) for p, kw in cases]
        assert want == [1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 0] and got == want, (got, want)
        assert 0 < st["max_input_sum_c2"] <= BUDGET and 20 < run.pbs < 700, run.pbs
    finally:
        run.close()


# ---- 5. the edges of the C ABI ----------------------------------------------------------------------------------------
def test_name_prototype_and_the_rust_binding(planner):
    from fhestring_amd import cabi
    header = cabi.parse_header()
    funcs, consts = {f[0]: f for f in header["funcs"]}, dict(header["consts"])
    assert "fhs_str_regex_clear" in funcs and "fhs_regex_info" in funcs
    assert (consts["FHS_REGEX_IGNORE_CASE"], consts["FHS_REGEX_SEARCH"], consts["FHS_REGEX_MAX_POSITIONS"]) == (1, 2, 64)
    f = planner.ctx._L.fhs_str_regex_clear
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p]
    g = planner.ctx._L.fhs_regex_info
    assert g.restype is C.c_int and g.argtypes == [C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(ROOT, "bindings", "fhestring_hip.rs")).read()
    assert "fn fhs_str_regex_clear(" in text and "fn fhs_regex_info(" in text and "FHS_REGEX_SEARCH" in text


def test_argument_errors_record_nothing(planner):
    from fhestring_amd import FhsError
    from fhestring_amd.api import _harr
    sk = planner
    L, h = sk.ctx._L, sk.ctx._h
    s = sk.dummy_string(5)
    gone = sk.dummy_string(1)[0]
    released = gone.h
    del gone
    sk.flush()
    st0 = sk.stats()
    arr, out = _harr(s.chars), (C.c_uint64 * 1)()
    bad_s = (C.c_uint64 * 5)(*[c.h for c in s.chars[:4]], released)
    rx = L.fhs_str_regex_clear
    bad = [("a null out", lambda: rx(h, arr, 5, b"ab", 2, 0, None)),
           ("a released handle", lambda: rx(h, bad_s, 5, b"ab", 2, 0, out)),
           ("unknown flag bits", lambda: rx(h, arr, 5, b"ab", 2, 4, out)),
           ("unknown flag bits beside the known ones", lambda: rx(h, arr, 5, b"ab", 2, 0x80000003, out)),
           ("a null pattern of length 2", lambda: rx(h, arr, 5, None, 2, 0, out)),
           ("a null context", lambda: rx(None, arr, 5, b"ab", 2, 0, out)),
           ("a null string of length 5", lambda: rx(h, None, 5, b"ab", 2, 0, out)),
           ("a NUL in the pattern", lambda: rx(h, arr, 5, b"a\0b", 3, 0, out))]
    for name, call in bad:
        assert call() == ERR_ARG, name
    with pytest.raises(FhsError) as err:
        sk.regex_clear(s, "a(b")
    assert err.value.code == ERR_ARG and "unbalanced" in str(err.value)
    assert rx(h, None, 0, None, 0, 0, out) == 0              # n == 0 and m == 0 need no pointers: "" on the empty text
    from fhestring_amd.api import FheAsciiChar
    assert FheAsciiChar(sk, out[0]).trivial_value() == 1
    sk.flush()
    assert sk.stats() == st0                                 # no node, no bootstrap, no block
    a, wa, _ = _flush_stats(sk, lambda: sk.regex_clear(s, b"a.*", ignore_case=True))       # bytes and str alike
    b, wb, _ = _flush_stats(sk, lambda: sk.regex_clear(s, "a.*", ignore_case=True))
    assert (a["pbs_executed"], a["pbs_extracted"], wa) == (b["pbs_executed"], b["pbs_extracted"], wb) and a["pbs_executed"] > 0
