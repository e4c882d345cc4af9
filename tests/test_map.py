"""map_clear, class_flags, find_class and their Python forms without a GPU:

* the logic by constant folding on a planner context against bytes.translate and Python's membership test: the named
  tables and classes of tools/gen_map_plan.py and seeded random ones on all 256 byte values, fused; the sparse ones as
  written;
* the bookkeeping on uploaded inputs: the to_upper table costs what to_upper costs, tables that change nothing cost
  nothing, the bounds per character, the noise budget with fresh and with the noisiest admitted operands, linear growth,
  and the pinned figures of tests/golden/map_plan.json;
* real ciphertexts through the CPU oracle's bootstrap (oracle/plan_exec.py);
* the edges of the C ABI and the Python forms."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_map_plan as gen  # noqa: E402

BUDGET = 64
ERR_ARG, ERR_LIMIT = -1, -4
ALL = bytes(range(256))


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


def _values(chars):
    return bytes(c.trivial_value() for c in chars)


def _members(sk, cls):
    bits = sk.class_set(cls)
    return [bits[v >> 3] >> (v & 7) & 1 for v in range(256)]


def py_find(buf, member, absent):
    return next((i for i, b in enumerate(buf) if member[b]), absent)


def _random_tables(n, seed):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        if k % 4 == 0:                                       # every byte anywhere
            out.append(bytes(rng.randrange(256) for _ in range(256)))
        elif k % 4 == 1:                                     # a permutation
            p = list(range(256))
            rng.shuffle(p)
            out.append(bytes(p))
        elif k % 4 == 2:                                     # a few changes to the identity
            t = bytearray(ALL)
            for _ in range(rng.randrange(1, 9)):
                t[rng.randrange(256)] = rng.randrange(256)
            out.append(bytes(t))
        else:                                                # structure in the nibbles: few distinct rows and columns
            f, g = [rng.randrange(4) for _ in range(16)], [rng.randrange(4) for _ in range(16)]
            out.append(bytes((f[v >> 4] * 4 + g[v & 15]) * 17 & 255 for v in range(256)))
    return out


def _random_sets(n, seed):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        if k % 3 == 0:
            out.append(bytes(v for v in range(256) if rng.random() < 0.5))
        elif k % 3 == 1:
            out.append(bytes(rng.sample(range(256), rng.randrange(1, 9))))
        else:
            lo = rng.randrange(256)
            out.append(bytes(range(lo, min(256, lo + rng.randrange(1, 80)))))
    return out


# ---- 1. folding ------------------------------------------------------------------------------------------------------
def test_fused_map_clear_folds_to_translate(folded):
    sk = folded
    sk.set_mode(1)
    s = _triv(sk, ALL)
    tables = list(gen.TABLES.items()) + [("random %d" % k, t) for k, t in enumerate(_random_tables(200, 0x3A9))]
    assert len(tables) == 208
    for name, table in tables:
        assert _values(sk.map_clear(s, table)) == ALL.translate(table), name
    assert sk.stats(reset=True)["pbs_executed"] == 0


def test_fused_classes_fold_to_membership(folded):
    sk = folded
    sk.set_mode(1)
    s = _triv(sk, ALL)
    classes = list(gen.CLASSES.items()) + [("random %d" % k, c) for k, c in enumerate(_random_sets(200, 0xC1A55))]
    for name, cls in classes:
        member = _members(sk, cls)
        assert list(_values(sk.class_flags(s, cls))) == member, name
    assert sum(_members(sk, gen.CLASSES["identifier"])) == 63 and sum(_members(sk, "^a-z")) == 230


@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256])
def test_find_class_on_buffers(folded, n):
    sk = folded
    rng = random.Random(n)
    classes = list(gen.CLASSES.values()) + _random_sets(12, 0xF1 + n)
    for mode in (1, 0):
        sk.set_mode(mode)
        for cls in classes:
            member = _members(sk, cls)
            if mode == 0 and (sum(member) > 8 or n > 17):    # as written: sparse sets, short buffers
                continue
            outside = [v for v in range(256) if not member[v]] or [0]
            inside = [v for v in range(256) if member[v]]
            for at in sorted({0, n // 2, n - 1, None}, key=lambda v: -1 if v is None else v):
                buf = bytearray(rng.choice(outside) for _ in range(n))
                if at is not None and inside:
                    buf[at] = rng.choice(inside)
                    if at + 1 < n:
                        buf[n - 1] = rng.choice(inside)      # a later member does not matter
                got = sk.find_class(_triv(sk, buf), cls).trivial_value()
                assert got == py_find(buf, member, 255), (mode, cls, n, at)
    sk.set_mode(1)


def test_find_class_wide_and_the_limits(folded):
    from fhestring_amd.api import FheU16
    sk = folded
    sk.set_mode(1)
    member = _members(sk, "0-9")
    for at in (0, 255, 256, 299, None):
        buf = bytearray(b"x" * 300)
        if at is not None:
            buf[at] = ord("7")
        got = sk.find_class_wide(_triv(sk, buf), "0-9")
        assert isinstance(got, FheU16)
        assert got.lo.trivial_value() + 256 * got.hi.trivial_value() == py_find(buf, member, 65535), at
    assert sk.find_class([], "0-9").trivial_value() == 255
    wide = sk.find_class_wide([], "0-9")
    assert (wide.lo.trivial_value(), wide.hi.trivial_value()) == (255, 255)
    with pytest.raises(OverflowError):
        sk.find_class(_triv(sk, b"x" * 257), "0-9")
    for mode in (1, 0):                                      # count_class and all_in_class, both modes
        sk.set_mode(mode)
        s = _triv(sk, b"ab1\0c23\0")
        n = sk.count_class(s, "0-3")
        assert n.lo.trivial_value() + 256 * n.hi.trivial_value() == 3
        assert sk.all_in_class(s, "a-c1-3").trivial_value() == 1 and sk.all_in_class(s, "a-c").trivial_value() == 0
    sk.set_mode(1)


def test_as_written_folds_on_sparse_tables(folded):
    sk = folded
    sk.set_mode(0)
    s = _triv(sk, ALL[::3] + b"0123456789azAZ")
    buf = bytes(ALL[::3] + b"0123456789azAZ")
    sparse = [t for t in list(gen.TABLES.values()) + _random_tables(40, 0x5A) if sum(a != b for a, b in zip(t, ALL)) <= 8]
    assert len(sparse) >= 10 and gen.TABLES["identity"] in sparse
    for table in sparse:
        assert _values(sk.map_clear(s, table)) == buf.translate(table)
    sets = [c for c in list(gen.CLASSES.values()) + _random_sets(40, 0x5B) if sum(_members(sk, c)) <= 8]
    assert len(sets) >= 10
    for cls in sets:
        member = _members(sk, cls)
        assert list(_values(sk.class_flags(s, cls))) == [member[b] for b in buf], cls
    sk.set_mode(1)


def test_class_specs_and_translate_forms(folded):
    sk = folded
    sk.set_mode(1)
    cs = sk.class_set
    assert cs("a-c") == cs(b"abc") == cs({97, 98, 99}) and cs("^") == b"\xff" * 32 and cs("") == bytes(32)
    assert cs("-a") == cs(b"-a") and cs("a-") == cs(b"a-") and cs("^^") == cs(set(range(256)) - {0x5E})
    assert cs("A-Za-z0-9_") == cs(set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_"))
    with pytest.raises(ValueError):
        cs("z-a")
    with pytest.raises(ValueError):
        cs({256})
    s = _triv(sk, b"a1-b2\0")
    assert _values(sk.translate(s, {"a": "x", ord("1"): b"#", b"-": 0})) == b"x#\0b2\0"
    assert _values(sk.translate(s, bytes.maketrans(b"ab", b"AB"))) == b"A1-B2\0"
    assert sk.in_class(s[1], "0-9").trivial_value() == 1 and _values(sk.in_class(s, "0-9")) == bytes([0, 1, 0, 0, 1, 0])
    with pytest.raises(ValueError):
        sk.map_clear(s, bytes(255))


# ---- 2. bookkeeping on uploaded inputs (fused) ----------------------------------------------------------------------
def _flush_stats(sk, fn):
    sk.flush()
    sk.stats(reset=True)
    keep = fn()
    sk.flush()
    return sk.stats(), keep


@pytest.mark.parametrize("n", gen.SIZES)
def test_the_case_tables_cost_what_the_built_ins_cost(planner, n):
    sk = planner
    s = sk.dummy_string(n)
    for table, built_in in ((gen.TABLES["to_upper"], sk.to_upper), (gen.TABLES["to_lower"], sk.to_lower)):
        a, _ = _flush_stats(sk, lambda: built_in(s))
        b, res = _flush_stats(sk, lambda: sk.map_clear(s, table))
        assert 0 < b["pbs_executed"] <= a["pbs_executed"] == 3 * n and b["levels"] <= a["levels"] == 2, (a, b)
        assert b["max_input_sum_c2"] <= a["max_input_sum_c2"] and max(c.sum_c2() for c in res) <= 4
        del res


@pytest.mark.parametrize("n", gen.SIZES)
def test_bounds_per_character_and_the_budget(planner, n):
    sk = planner
    s = sk.dummy_string(n)
    for name, table in list(gen.TABLES.items()) + [("random %d" % k, t) for k, t in enumerate(_random_tables(12, 0xB0))]:
        st, res = _flush_stats(sk, lambda: sk.map_clear(s, table))
        assert st["pbs_executed"] <= 192 * n and st["max_input_sum_c2"] <= BUDGET, (name, st)
        if name in ("identity", "constant"):
            assert st["pbs_executed"] == 0 and st["pbs_folded"] == 0, name
        else:
            assert st["pbs_executed"] > 0 and max(c.sum_c2() for c in res) <= 4, name
        del res
    for name, cls in list(gen.CLASSES.items()) + [("random %d" % k, c) for k, c in enumerate(_random_sets(12, 0xB1))]:
        st, res = _flush_stats(sk, lambda: sk.class_flags(s, cls))
        assert st["pbs_executed"] <= 49 * n and st["max_input_sum_c2"] <= BUDGET and max(c.sum_c2() for c in res) <= 4, (name, st)
        if name == "lower":
            assert st["pbs_executed"] <= 3 * n
        if name in ("empty", "full"):
            assert st["pbs_executed"] == 0
        del res
    st, res = _flush_stats(sk, lambda: sk.find_class(s, "0-9"))
    assert 3 * n < st["pbs_executed"] and st["max_input_sum_c2"] <= BUDGET
    del res


def test_noisy_operands_stay_within_the_budget(planner):
    """operands at the largest figure an operand comes in with (4: above that, loading refreshes), declared with
    set_noise, and operands that are results: the nibble packing refreshes where 17 times the figure leaves the budget"""
    sk = planner
    declared = sk.dummy_string(16)
    for c in declared.chars:
        c.set_noise(4)
    folded_case = sk.to_upper(sk.dummy_string(16))
    mapped = sk.map_clear(sk.dummy_string(16), gen.TABLES["rot13"])
    sk.flush()
    assert max(c.sum_c2() for c in mapped) == 3
    for operand in (declared, folded_case, mapped):
        for table in (gen.TABLES["to_upper"], gen.TABLES["rot13"], gen.TABLES["random"], gen.TABLES["bit_reversal"]):
            st, res = _flush_stats(sk, lambda: sk.map_clear(operand, table))
            assert 0 < st["max_input_sum_c2"] <= BUDGET and max(c.sum_c2() for c in res) <= 4, st
            del res
        for cls in ("a-z", "A-Za-z0-9_"):
            st, res = _flush_stats(sk, lambda: sk.find_class(operand, cls))
            assert 0 < st["max_input_sum_c2"] <= BUDGET, st
            del res


@pytest.mark.parametrize("name", ["to_upper", "rot13", "random"])
def test_cost_is_linear(name):
    a, b = gen.measure_map(name, 16), gen.measure_map(name, 64)
    assert b["pbs_executed"] == 4 * a["pbs_executed"] > 0 and b["levels"] == a["levels"]
    a, b = gen.measure_class("identifier", 16), gen.measure_class("identifier", 64)
    assert b["pbs_executed"] == 4 * a["pbs_executed"] > 0 and b["levels"] == a["levels"]


def test_pinned_plan():
    with open(gen.PATH) as f:
        pinned = json.load(f)
    assert gen.generate() == pinned
    assert len(pinned["map_clear"]) == 2 * len(gen.TABLES) and len(pinned["class_flags"]) == 2 * len(gen.CLASSES)


# ---- 3. real ciphertexts, the CPU oracle's bootstrap ----------------------------------------------------------------
def test_results_decrypt_on_real_ciphertexts(oracle_keys, oracle_sk):
    from oracle.plan_exec import PlanRun
    K = oracle_keys
    run = PlanRun(oracle_sk, threads=min(16, os.cpu_count() or 1), mode=6)
    try:
        sk = run.sk
        buf = b"Az7\0"
        s = run.upload_string(np.stack([K.encrypt_char(b) for b in buf]))
        rot, digits = sk.map_clear(s, gen.TABLES["rot13"]), sk.class_flags(s, "0-9")
        run.run()
        st = sk.stats()
        assert bytes(K.decrypt_char(run.result_char(ch)) for ch in rot) == buf.translate(gen.TABLES["rot13"]) == b"Nm7\0"
        assert [K.decrypt_char(run.result_char(ch)) for ch in digits] == [0, 0, 1, 0]
        assert 0 < st["max_input_sum_c2"] <= BUDGET and 0 < run.pbs <= 4 * (18 + 3)       # ROT13's 18 per character, the class's 3
    finally:
        run.close()


# ---- 4. the edges of the C ABI ----------------------------------------------------------------------------------------
def test_names_prototypes_and_the_rust_binding(planner):
    from fhestring_amd import cabi
    funcs = {f[0] for f in cabi.parse_header()["funcs"]}
    names = ("fhs_user_lut", "fhs_debug_read_lut", "fhs_str_map_clear", "fhs_str_class_flags", "fhs_str_find_class",
             "fhs_str_find_class_wide")
    assert funcs.issuperset(names)
    L = planner.ctx._L
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    assert (L.fhs_user_lut.restype, L.fhs_user_lut.argtypes) == (i, [vp, vp])
    assert (L.fhs_debug_read_lut.restype, L.fhs_debug_read_lut.argtypes) == (i, [vp, i, vp])
    for name in names[2:5]:
        assert (getattr(L, name).restype, getattr(L, name).argtypes) == (i, [vp, vp, sz, vp, vp]), name
    assert L.fhs_str_find_class_wide.argtypes == [vp, vp, sz, vp, vp, vp]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(ROOT, "bindings", "fhestring_hip.rs")).read()
    for name in names:
        assert "fn %s(" % name in text, name
    assert "fn fhs_str_map_clear(c: *mut fhs_ctx, s: *const fhs_char_t, n: usize, table: *const u8" in text


def test_argument_errors_record_nothing(planner):
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
    st0, tables0 = sk.stats(), L.fhs_user_lut_count()
    arr, out, hi = _harr(s.chars + [noisy]), (C.c_uint64 * 6)(), (C.c_uint64 * 1)()
    bad_s = (C.c_uint64 * 5)(*[c.h for c in s.chars[:4]], released)
    table, bits = bytes(reversed(range(256))), bytes([0x5A] * 32)             # neither has been planned in this process
    bad = [("map: a null table", lambda: L.fhs_str_map_clear(h, arr, 6, None, out)),
           ("map: a null out", lambda: L.fhs_str_map_clear(h, arr, 6, table, None)),
           ("map: a null string", lambda: L.fhs_str_map_clear(h, None, 6, table, out)),
           ("map: a null context", lambda: L.fhs_str_map_clear(None, arr, 6, table, out)),
           ("map: a released handle", lambda: L.fhs_str_map_clear(h, bad_s, 5, table, out)),
           ("flags: a null set", lambda: L.fhs_str_class_flags(h, arr, 6, None, out)),
           ("flags: a null out", lambda: L.fhs_str_class_flags(h, arr, 6, bits, None)),
           ("flags: a released handle", lambda: L.fhs_str_class_flags(h, bad_s, 5, bits, out)),
           ("find: a null set", lambda: L.fhs_str_find_class(h, arr, 6, None, out)),
           ("find: a null out", lambda: L.fhs_str_find_class(h, arr, 6, bits, None)),
           ("find: a null out for no characters", lambda: L.fhs_str_find_class(h, None, 0, bits, None)),
           ("find: a null string", lambda: L.fhs_str_find_class(h, None, 6, bits, out)),
           ("wide: a null hi", lambda: L.fhs_str_find_class_wide(h, arr, 6, bits, out, None)),
           ("wide: a null lo", lambda: L.fhs_str_find_class_wide(h, arr, 6, bits, None, hi)),
           ("wide: a released handle", lambda: L.fhs_str_find_class_wide(h, bad_s, 5, bits, out, hi))]
    for name, call in bad:
        assert call() == ERR_ARG, name
    long_arr = _harr(s.chars * 52)                           # 260 handles: past the u8 form's reach, checked first
    assert L.fhs_str_find_class(h, long_arr, 260, bits, out) == ERR_LIMIT
    sk.flush()
    assert sk.stats() == st0 and L.fhs_user_lut_count() == tables0         # no node, no bootstrap, no block, no table


def test_empty_strings(planner):
    from fhestring_amd.api import FheAsciiChar
    sk = planner
    L, h = sk.ctx._L, sk.ctx._h
    st0 = sk.stats()
    for mode in (0, 1):
        sk.set_mode(mode)
        assert len(sk.map_clear([], gen.TABLES["rot13"])) == 0 and len(sk.class_flags([], "a-z")) == 0
        assert L.fhs_str_map_clear(h, None, 0, gen.TABLES["rot13"], None) == 0      # n == 0 needs no pointers
        assert L.fhs_str_class_flags(h, None, 0, bytes(32), None) == 0
        out = (C.c_uint64 * 1)()
        assert L.fhs_str_find_class(h, None, 0, bytes(32), out) == 0
        assert FheAsciiChar(sk, out[0]).trivial_value() == 255
    sk.set_mode(1)
    sk.flush()
    assert sk.stats() == st0
