#!/usr/bin/env python3
"""Plan digests of the string layer (tests/golden/strings_digests.json, checked by tests/test_strings_digest.py).

tools/gen_plan_digests.py pins the scheduler on a few large operations; this fixture pins what the string layer RECORDS:
every entry point that fhestring_amd/csrc/capi_ops.cpp wraps, at the smallest shapes at which each of its paths can
still go wrong, in as-written and fused mode (suffix _aw / _f).  A digest is gen_plan_digests.record(): plan trace,
result terms, statistics, level widths and launch groups of one scenario on a planner context (no GPU); a scenario that
ends in an error digests the error code with what was recorded up to it.

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


def main():
    out = {name: fn() for name, fn in SCENARIOS.items()}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d digests to %s" % (len(out), os.path.relpath(FIXTURE, ROOT)))


if __name__ == "__main__":
    main()
