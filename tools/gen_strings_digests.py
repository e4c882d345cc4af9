#!/usr/bin/env python3
"""Plan digests of the string layer (tests/golden/strings_digests.json, checked by tests/test_strings_digest.py).

tools/gen_plan_digests.py pins the scheduler on a few large operations; this fixture pins what the string layer RECORDS:
every entry point that fhestring_amd/csrc/capi_ops.cpp wraps, at the smallest shapes at which each of its paths can
still go wrong, in as-written and fused mode (suffix _aw / _f).  A digest is gen_plan_digests.record(): plan trace,
result terms, statistics, level widths and launch groups of one scenario on a planner context (no GPU); a scenario that
ends in an error digests the error code with what was recorded up to it.

Sections 7 to 10 pin the pattern languages -- like_clear, map_clear / class_flags / find_class, regex_clear and
regex_find_clear / regex_starts_clear.  Fused, these apply user tables, whose ids are process-wide; record() renames them
by first appearance within the scenario and hashes their contents, so a digest is the same whatever the process
registered before: alone, in this file's order, or in pytest's sorted order.

The fixture was recorded from the library as it was BEFORE the string layer was refactored and is not regenerated for
a change that only moves code: a digest that moves means that an entry point records other rows, or the same rows in
another order.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_plan_digests import record  # noqa: E402  (puts ROOT on sys.path)

FIXTURE = os.path.join(ROOT, "tests", "golden", "strings_digests.json")
CLEAR = "a2S$xy"                       # clear patterns are its prefixes
MODES = ((0, "aw"), (1, "f"))
SCENARIOS = {}


def add(name, body, modes=MODES):
    for mode, tag in modes:
        key = "%s_%s" % (name, tag)
        assert key not in SCENARIOS, key
        SCENARIOS[key] = lambda body=body, mode=mode: record(body, mode=mode)


FUSED = MODES[1:]


# ---- 1. producers: every shape in both modes; 2. the digit boundaries of the fused forms ----
def _pat_op(op, n, m):
    if "clear" in op:
        return lambda sk: getattr(sk, op)(sk.dummy_string(n), CLEAR[:m])
    return lambda sk: getattr(sk, op)(sk.dummy_string(n), sk.dummy_string(m))


def _str_op(op, n):
    return lambda sk: getattr(sk, op)(sk.dummy_string(n))


PAT_OPS = ("find", "find_clear", "rfind", "find_wide", "find_clear_wide", "rfind_wide")
STR_OPS = ("len", "len_wide", "count_flags_wide")
SHAPES = ((0, 0), (1, 0), (0, 1), (1, 1), (5, 2), (5, 5), (5, 6), (17, 3), (70, 4))
for _n, _m in SHAPES:
    for _op in PAT_OPS:
        add("%s_%d_%d" % (_op, _n, _m), _pat_op(_op, _n, _m))
for _n in sorted({n for n, _ in SHAPES}):
    for _op in STR_OPS:
        add("%s_%d" % (_op, _n), _str_op(_op, _n))
for _n in (5, 17):                     # the empty pattern is a branch of its own in rfind
    for _op in ("rfind", "rfind_wide"):
        add("%s_empty_%d" % (_op, _n), _pat_op(_op, _n, 0))
for _n in (4, 5, 16, 17, 64, 65):      # first_index and count_flags change shape where W or n crosses a power of four
    for _op in ("find", "find_wide"):
        add("%s_%d_1" % (_op, _n), _pat_op(_op, _n, 1), FUSED)
    for _op in ("len", "len_wide"):
        if _n not in (5, 17):
            add("%s_%d" % (_op, _n), _str_op(_op, _n), FUSED)
add("find_256_2", _pat_op("find", 256, 2), FUSED)             # W = 255, the most the u8 form allows
for _n in (257, 1025):                                        # digit 4 and digit 5 become live
    for _op in ("find_wide", "rfind_wide"):
        add("%s_%d_3" % (_op, _n), _pat_op(_op, _n, 3), FUSED)
    add("len_wide_%d" % _n, _str_op("len_wide", _n), FUSED)

# ---- 3. limits ----
add("limit_find_255_0", _pat_op("find", 255, 0))              # FHS_ERR_LIMIT
add("limit_rfind_254_0", _pat_op("rfind", 254, 0))            # FHS_ERR_LIMIT: the NUL that rfind pushes counts
add("limit_find_254_0", _pat_op("find", 254, 0))              # the longest string find takes


def _noisy_first(sk, n, repeat):
    """a string whose first char is find's result (index digits: sum c^2 > 4, refreshed when loaded as an operand)"""
    r = sk.find(sk.dummy_string(17), sk.dummy_string(3))
    return [r] * n if repeat else [r] + sk.dummy_string(n - 1).chars


# the u8 forms load their operands before the limit test (the refresh is recorded), the wide forms test first
add("limit_order_find", lambda sk: sk.find(_noisy_first(sk, 255, False), []), FUSED)
add("limit_order_find_wide", lambda sk: sk.find_wide(_noisy_first(sk, 65535, True), []), FUSED)   # one handle, 65535 times


# ---- 4. consumers of a position ----
def _pos(sk, kind):
    from fhestring_amd.api import FheU16
    if kind == "u8":
        return sk.dummy_string(1)[0]
    lo, hi = sk.dummy_string(2).chars
    return FheU16(lo, hi)


def _consumer(op, n, kind, count=None):
    if op == "substr":
        return lambda sk: sk.substr(sk.dummy_string(n), _pos(sk, kind), count)
    return lambda sk: getattr(sk, op)(sk.dummy_string(n), _pos(sk, kind))


for _n in (1, 5, 17, 64, 65):
    for _kind in ("u8", "wide"):
        for _op in ("char_at", "take", "split_at"):
            add("%s_%s_%d" % (_op, _kind, _n), _consumer(_op, _n, _kind))
        for _count in sorted({1, 3, _n, _n + 5}):
            add("substr_%s_%d_%d" % (_kind, _n, _count), _consumer("substr", _n, _kind, _count))


def _char_at_find(sk):
    s = sk.dummy_string(17)
    return sk.char_at(s, sk.find(s, sk.dummy_string(3)))


def _substr_find_wide(sk):
    s = sk.dummy_string(17)
    return sk.substr(s, sk.find_wide(s, sk.dummy_string(3)), 3)


add("char_at_of_find_17_3", _char_at_find, FUSED)             # the digit refresh of load and pos_digits
add("substr_of_find_wide_17_3", _substr_find_wide, FUSED)


# ---- 5. folding: trivial chars ----
def _text(sk, n, every=1):
    """n chars, trivial at every `every`-th index"""
    d = sk.dummy_string(n).chars
    return [sk.trivial(97 + i % 3) if i % every == 0 else d[i] for i in range(n)]


for _tag, _every in (("trivial", 1), ("half_trivial", 2)):
    add("find_clear_%s_9" % _tag, lambda sk, e=_every: sk.find_clear(_text(sk, 9, e), "ab"))
    add("rfind_empty_%s_9" % _tag, lambda sk, e=_every: sk.rfind(_text(sk, 9, e), []))
    add("len_%s_9" % _tag, lambda sk, e=_every: sk.len(_text(sk, 9, e)))
add("count_flags_wide_same_flag_20", lambda sk: sk.count_flags_wide([sk.dummy_string(1)[0]] * 20))   # counted in halves
add("char_at_trivial_pos_17", lambda sk: sk.char_at(sk.dummy_string(17), sk.trivial(3)))


# ---- 6. every other family of capi_ops.cpp, once, at (5, 2) ----
def _two(op, n=5, m=2):
    return lambda sk: getattr(sk, op)(sk.dummy_string(n), sk.dummy_string(m))


for _op in ("contains", "starts_with", "ends_with", "eq", "ne", "eq_ignore_case", "lt", "le", "gt", "ge", "concatenate",
            "strip_prefix", "strip_suffix", "split", "split_inclusive", "split_terminator", "rsplit", "rsplit_terminator",
            "rsplit_once"):
    add("%s_5_2" % _op, _two(_op))
for _op in ("splitn", "rsplitn"):
    add("%s_5_2" % _op, lambda sk, op=_op: getattr(sk, op)(sk.dummy_string(5), sk.dummy_string(2), sk.dummy_string(1)[0]))
add("split_ascii_whitespace_5", _str_op("split_ascii_whitespace", 5))
add("compare_partial_5_5", lambda sk: sk.compare_partial(sk.dummy_string(5), sk.dummy_string(5), 1))
for _tie in (0, 1):
    add("flags_first_decides_3_tie%d" % _tie,
        lambda sk, tie=_tie: sk.flags_first_decides(sk.dummy_string(3).chars, sk.dummy_string(3).chars, tie))
for _op in ("to_upper", "to_lower", "trim", "trim_start", "trim_end", "bubble_zeroes_right", "flags_or", "flags_and"):
    add("%s_5" % _op, _str_op(_op, 5))
add("replace_5_2_1", lambda sk: sk.replace(sk.dummy_string(5), sk.dummy_string(2), sk.dummy_string(1)))
add("replace_5_1_2", lambda sk: sk.replace(sk.dummy_string(5), sk.dummy_string(1), sk.dummy_string(2)))
add("replacen_5_2_1", lambda sk: sk.replacen(sk.dummy_string(5), sk.dummy_string(2), sk.dummy_string(1), sk.dummy_string(1)[0]))
add("repeat_5", lambda sk: sk.repeat(sk.dummy_string(5), sk.dummy_string(1)[0]))
add("repeat_clear_5_2", lambda sk: sk.repeat_clear(sk.dummy_string(5), 2))


# ---- 7. LIKE against clear patterns ----
def _like(n, pattern, **kw):
    return lambda sk: sk.like_clear(sk.dummy_string(n), pattern, **kw)


LIKE = (("empty", "", {}), ("any", "%", {}), ("lit", "a", {}), ("one", "_", {}), ("anchored", "a_%", {}),
        ("contains", "%ab%", {}), ("middle", "a%b%c", {}),                 # a middle segment: the inclusive prefix OR
        ("any_any", "%%a", {}), ("ilike", "%aB%", {"ignore_case": True}),
        ("escape", "a!%%!_b", {"escape": "!"}),                            # the literals % and _ around an ANY
        ("refused", "ab!", {"escape": "!"}))                               # a dangling escape: FHS_ERR_ARG
for _tag, _pattern, _kw in LIKE:
    for _n in (0, 1, 5, 17):
        add("like_%s_%d" % (_tag, _n), _like(_n, _pattern, **_kw))
for _n in (9, 17):                     # 16 nibble flags and extras: the chunked AND of the window
    add("like_window16_%d" % _n, _like(_n, "%abcdefgh"))
add("like_half_trivial_17", lambda sk: sk.like_clear(_text(sk, 17, 2), "%ab%c"))


# ---- 8. clear tables and classes ----
def _tables():
    import gen_map_plan
    return gen_map_plan.TABLES, gen_map_plan.CLASSES


def _map(n, name):
    return lambda sk: sk.map_clear(sk.dummy_string(n), _tables()[0][name])


def _class(op, n, name):
    return lambda sk: getattr(sk, op)(sk.dummy_string(n), b"a" if name == "one_byte" else _tables()[1][name])


for _n in (1, 5):
    # identity: PASS; constant: CONST; to_upper: one table on a digit; the others factor into PICK and LINES plans
    for _name in ("identity", "constant", "to_upper", "mask_digits", "rot13", "bit_reversal", "random"):
        add("map_clear_%s_%d" % (_name, _n), _map(_n, _name))
    for _name in ("one_byte", "digits", "hex", "identifier", "whitespace"):   # one byte, a range, sets that need LINES
        for _op in ("class_flags", "find_class"):
            add("%s_%s_%d" % (_op, _name, _n), _class(_op, _n, _name))
for _op in ("find_class", "find_class_wide"):
    add("%s_identifier_17" % _op, _class(_op, 17, "identifier"))
add("limit_find_class_257", _class("find_class", 257, "digits"))


# ---- 9. regular expressions against clear patterns ----
def _regex(op, n, pattern, **kw):
    return lambda sk: getattr(sk, op)(sk.dummy_string(n), pattern, **kw)


REGEX = (("abc", b"abc", {}),                                              # BYTE classes; a literal costs L steps
         ("a_icase", b"a", {"ignore_case": True}), ("dot", b".", {}), ("table", b"[a-c]x", {}),
         ("dead", rb"a\0", {}), ("nullable", b"a*", {}),
         ("preds", b"(ab|c)+d", {}),                                       # k >= 2 predecessors: a threshold table
         ("search", b"ab", {"search": True}), ("search_preds", b"(ab|c)+d", {"search": True}))
for _tag, _pattern, _kw in REGEX:
    for _n in (0, 1, 5, 17):
        add("regex_%s_%d" % (_tag, _n), _regex("regex_clear", _n, _pattern, **_kw))
add("regex_five_preds_5", _regex("regex_clear", 5, b"(a|b|c|d|e)+f"))      # 6 * 2 + 5 > 15: or_tree first in regex_step
add("regex_half_trivial_17", lambda sk: sk.regex_clear(_text(sk, 17, 2), b"a+"))
add("regex_refused", _regex("regex_clear", 5, b"a$"))

# ---- 10. where a regular expression matches ----
FIND_OPS = (("regex_find", "regex_find_clear"), ("regex_find_wide", "regex_find_clear_wide"), ("regex_starts", "regex_starts_clear"))
for _tag, _pattern in (("abc", b"abc"), ("nullable", b"a*"), ("table", b"[a-c]+x"), ("preds", b"(ab|c)+d")):
    for _n in (0, 1, 5, 17):
        for _name, _op in FIND_OPS:
            add("%s_%s_%d" % (_name, _tag, _n), _regex(_op, _n, _pattern))
for _name, _op in FIND_OPS:
    for _tag, _pattern in (("byte", b"a+x"), ("table", b"[a-c]+x")):
        add("%s_half_trivial_%s_17" % (_name, _tag), lambda sk, op=_op, p=_pattern: getattr(sk, op)(_text(sk, 17, 2), p))
add("limit_regex_find_257", _regex("regex_find_clear", 257, b"abc"))


def main():
    out = {name: fn() for name, fn in SCENARIOS.items()}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d digests to %s" % (len(out), os.path.relpath(FIXTURE, ROOT)))


if __name__ == "__main__":
    main()
