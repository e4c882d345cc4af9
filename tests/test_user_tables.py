"""User look-up tables beside the catalogue, host side: the process-wide registry behind
fhs_user_lut, interning, the ids, the polynomials fhs_debug_lut_poly answers with, folding through the padding-bit rule,
the capacity, and that the catalogue is where it was.  No GPU: the device copies are checked by tests/test_map_device.py."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE, ERR_LIMIT = -1, -3, -4
N, BOX = 2048, 128


def lut_poly_py(values):
    """make_lut_poly restated: 16 boxes of 128 holding value << 59, rotated left by half a box, the wrapped part negated"""
    tmp = np.repeat(np.array([v & 31 for v in values], np.uint64) << np.uint64(59), BOX)
    return np.concatenate([tmp[BOX // 2:], (np.uint64(0) - tmp[:BOX // 2])])


@pytest.fixture(scope="module")
def L():
    import fhestring_amd
    return fhestring_amd.lib()


def register(L, values):
    out = C.c_int(-1)
    rc = L.fhs_user_lut(bytes(values), C.byref(out))
    return rc, out.value


def poly(L, lut_id):
    out = np.zeros(N, np.uint64)
    assert L.fhs_debug_lut_poly(int(lut_id), out.ctypes.data_as(C.c_void_p)) == 0, lut_id
    return out


def test_the_restatement_is_the_oracles_polynomial():
    from oracle import radix
    for name in ("msg", "sel_t", "cmp_le"):
        assert np.array_equal(lut_poly_py([radix.LUTS[name](v) for v in range(16)]), radix.lut_poly(name)), name


def test_registered_tables_answer_with_their_polynomial(L):
    rng = random.Random(0x7AB)
    n_cat = L.fhs_lut_catalogue_count()
    tables = [[rng.randrange(32) for _ in range(16)] for _ in range(64)]
    tables[0] = [31] * 16                                    # every value negative: the wrapped part is +1 << 59
    tables[1] = [0] * 15 + [17]
    ids = []
    for t in tables:
        rc, i = register(L, t)
        assert rc == 0 and n_cat <= i < 65536, (rc, i)
        ids.append(i)
    assert len(set(ids)) == len(set(map(tuple, tables)))
    for t, i in zip(tables, ids):
        assert np.array_equal(poly(L, i), lut_poly_py(t)), t
    count = L.fhs_user_lut_count()
    assert [register(L, t) for t in tables] == [(0, i) for i in ids]          # interned: equal content, equal id
    assert L.fhs_user_lut_count() == count
    fresh = [rng.randrange(32) for _ in range(16)]
    fresh[3] = 29
    rc, i = register(L, fresh)
    if L.fhs_user_lut_count() == count + 1:                  # (not met before in this process)
        assert (rc, i) == (0, n_cat + count)                 # ids count up in order of first registration


def test_argument_errors_register_nothing(L):
    count = L.fhs_user_lut_count()
    out = C.c_int(-7)
    assert L.fhs_user_lut(None, C.byref(out)) == ERR_ARG
    assert L.fhs_user_lut(bytes(16), None) == ERR_ARG
    assert L.fhs_user_lut(bytes([0] * 15 + [32]), C.byref(out)) == ERR_ARG and out.value == -7
    assert L.fhs_user_lut_count() == count
    buf = np.zeros(N, np.uint64)
    n_cat = L.fhs_lut_catalogue_count()
    assert L.fhs_debug_lut_poly(n_cat + count, buf.ctypes.data_as(C.c_void_p)) == ERR_ARG        # not registered
    assert L.fhs_debug_lut_poly(-1, buf.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert L.fhs_debug_lut_poly(0, None) == ERR_ARG


def test_the_catalogue_is_where_it_was(L):
    """ids 0 .. 22 are the tables the oracle knows by name, in the order of the enum; the count is the parent's"""
    from oracle import radix
    names = ["eq_biv", "ne_biv", "and_biv", "or_biv", "is4", "nz", "msg", "carry", "sign", "cmp_lt", "cmp_le", "cmp_gt",
             "cmp_ge", "sel_t", "sel_f"] + ["eq_c%d" % c for c in range(4)] + ["ne_c%d" % c for c in range(4)]
    assert sorted(names) == sorted(radix.LUTS)
    for i, name in enumerate(names):
        assert np.array_equal(poly(L, i), radix.lut_poly(name)), name
    n_cat = L.fhs_lut_catalogue_count()
    assert n_cat == 71
    for i in range(n_cat):                                   # every catalogue table has a 16-box polynomial of block values
        p = poly(L, i)
        assert np.array_equal(p, lut_poly_py([int(v) >> 59 for v in np.concatenate([np.uint64(0) - p[-64:], p])[::BOX][:16]])), i


def test_folding_uses_the_padding_bit_rule_on_a_user_table():
    """a planner context folds a bootstrap of a plaintext block through lut_eval: class_flags of a one-member set on a
    trivial character is the table's value, and the registry is what both modes and every context share"""
    from fhestring_amd.api import MyServerKey
    a, b = MyServerKey.planner(), MyServerKey.planner()
    try:
        for sk in (a, b):
            sk.set_mode(1)
            assert [sk.in_class(sk.trivial(v), b"k").trivial_value() for v in (0x6B, 0x6A, 0x7B, 0)] == [1, 0, 0, 0]
            assert sk.stats()["pbs_executed"] == 0 and sk.stats()["pbs_folded"] > 0
    finally:
        a.close()
        b.close()


def test_a_planner_context_has_no_device_tables():
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.planner()
    try:
        buf = np.zeros(N, np.uint64)
        Lp = sk.ctx._L
        assert Lp.fhs_debug_read_lut(sk.ctx._h, 0, buf.ctypes.data_as(C.c_void_p)) == ERR_STATE
        assert Lp.fhs_debug_read_lut(sk.ctx._h, 0, None) == ERR_ARG
        assert Lp.fhs_debug_read_lut(None, 0, buf.ctypes.data_as(C.c_void_p)) == ERR_ARG
    finally:
        sk.close()


_FILL = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
import fhestring_amd
L = fhestring_amd.lib()
cap = 65536 - L.fhs_lut_catalogue_count()
out = C.c_int()
for k in range(cap):
    t = bytes((k >> (5 * j)) & 31 for j in range(4)) + bytes(12)
    assert L.fhs_user_lut(t, C.byref(out)) == 0, k
assert out.value == 65535 and L.fhs_user_lut_count() == cap
out.value = -7
assert L.fhs_user_lut(bytes([1] * 16), C.byref(out)) == -4 and out.value == -7      # full: an error, nothing recorded
assert L.fhs_user_lut_count() == cap
assert L.fhs_user_lut(bytes(16), C.byref(out)) == 0 and out.value == L.fhs_lut_catalogue_count()   # known content still answers
from fhestring_amd.api import MyServerKey
sk = MyServerKey.planner()
sk.set_mode(1)
s = sk.dummy_string(2)
sk.flush()
st = sk.stats()
try:
    sk.map_clear(s, bytes(range(1, 256)) + b"\0")
    raise SystemExit("map_clear with a full registry must fail")
except OverflowError:
    pass
except Exception as e:
    assert getattr(e, "code", None) == -4, e
sk.flush()
assert sk.stats() == st
print("ok")
"""


def test_registration_past_the_capacity_is_refused():
    """in a process of its own: the registry is append-only, a full one would starve every test behind this one"""
    r = subprocess.run([sys.executable, "-c", _FILL % ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
