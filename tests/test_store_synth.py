"""The host references of the string store's GLWE keyswitch family (fhs_rekey_host, fhs_rekey_packed_host,
fhs_store_packed_host, fhs_store_select_host) under synthetic keys and on chosen words, against tests/store_model.py:
integer numpy with no product through a transform and no call into the library.  Every comparison is exact word
equality.

    identity key      K[l] = (-g_l X^m, 0): the re-key returns X^m mask and the body itself, in all three formats
    monomial keys     every key polynomial is one word times X^e: a signed roll of the digit polynomial times a word; the
                      key words put the keyswitch sum on the ties and wraps of round32 and round16 AFTER the sum
    gadget queries    the noise-free GGSW of every index bit: the select returns the words of the source row itself, or
                      zeros where the tree has no node -- the select's index arithmetic in closed form
    monomial queries  the CMux tree and the rotates as a recursion on 2048-vectors
    dense, extreme    schoolbook products under keys from the extremes of the grid rounding, and the all -2^15 case at the
                      top of the exact range
    controls          the model with ONE formula wrong differs from the reference on these inputs: the inputs are sensitive

About two in three input words are chosen (store_model.MASK_WORDS and its neighbours); how often a run reaches each
boundary is counted by the model and printed (pytest -s).  tests/test_store_synth_device.py runs the same inputs through
the kernels."""
import dataclasses
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import store_model as sm
from ring_util import digits32

N = 2048
U64 = np.uint64
CONTROL_BLOCKS = 2052                                       # two groups, the second of four blocks
CONTROL_CHARS = 513


def _same(got, want, what):
    for g, w, name in zip(got, want, ("mask", "body")):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        assert np.array_equal(g, w), "%s: %s, %d words differ" % (name, what, int((g != w).sum()))


def _raw(p):
    """(mask16, body16) of a PackedFheString or of the raw pair of a block count that is no multiple of 4"""
    return p if isinstance(p, tuple) else (p.mask16, p.body16)


def _all_reached(tally, what):
    print("boundaries reached, %s:\n%s" % (what, tally))
    assert tally.counts and all(hits > 0 for hits in tally.counts.values()), tally.counts


@pytest.fixture(scope="module")
def specs():
    return sm.rekey_specs()


def _compact(n_chars):
    from fhestring_amd.api import CompactFheString
    return CompactFheString(n_chars, *sm.entry_words(n_chars))


# ---- re-key ------------------------------------------------------------------------------------------------------------
def test_the_models_digits_are_ring_utils():
    w = np.concatenate([sm.MASK_WORDS, np.arange(0x7FFE, 0x8003, dtype=np.uint32) << np.uint32(16),
                        np.random.default_rng(0).integers(0, 1 << 32, 4096, dtype=np.uint32)])
    for mine, theirs in zip(sm.digits2(w), digits32(w)):
        assert np.array_equal(mine, theirs)
    assert all(hits > 0 for hits in sm.digit_classes(sm.MASK_WORDS).values())


def test_identity_key_returns_its_input():
    from fhestring_amd.api import rekey_host, rekey_packed_host, store_packed_host
    key = sm.rekey_key(sm.identity_key())
    for n_blocks in sm.BLOCK_COUNTS:
        mask, body = sm.rekey_words(n_blocks)
        _same(rekey_host(key, mask, body, n_blocks), (mask, body), ("identity", n_blocks))
        m64, b64 = sm.packed_words(n_blocks)
        want = sm.round16(sm.round32(m64).astype(U64) << U64(32)), sm.round16(b64).reshape(-1)[:n_blocks]
        _same(_raw(rekey_packed_host(key, m64, b64, n_blocks)), want, ("identity, packed", n_blocks))
    mask, body = sm.rekey_words(2052)
    for m in (5, 1024, 2047):                                # X^m mask: a roll to the right, negated where it wraps
        want = np.roll(mask, m, axis=1)
        want[:, :m] = np.uint32(0) - want[:, :m]
        _same(rekey_host(sm.rekey_key(sm.identity_key(m)), mask, body, 2052), (want, body), ("identity X^%d" % m,))
    for n_chars in sm.WINDOW_CHARS:
        c = _compact(n_chars)
        for first, count in sm.windows(n_chars):
            own, ident = store_packed_host(None, c, first, count), store_packed_host(key, c, first, count)
            assert own.first_coef == ident.first_coef
            _same(_raw(ident), _raw(own), ("identity against the own-key switch", n_chars, first, count))
            _same(_raw(own), sm.store_packed(None, c.mask32, c.body32, 4 * n_chars, first, count)[:2], ("own key", n_chars, first, count))


def test_monomial_keys_equal_the_model(specs):
    from fhestring_amd.api import rekey_host, rekey_packed_host, store_packed_host
    assert len(specs) >= 4
    assert {w for s in specs.values() for row in s for w, _ in row} >= set(sm.KEY_WORDS)
    total = sm.Tally()
    for name, spec in specs.items():
        assert {e for row in spec for _, e in row} == set(sm.EXPONENTS)
        key = sm.rekey_key(spec)
        total.add(sm.pm.key_classes([w for row in spec for w, _ in row]))
        for n_blocks in sm.BLOCK_COUNTS:
            mask, body = sm.rekey_words(n_blocks)
            assert np.isin(mask, sm.MASK_WORDS).mean() >= 0.6 or n_blocks < 100
            _same(rekey_host(key, mask, body, n_blocks), sm.rekey(spec, mask, body, n_blocks, tally=total), ("re-key", name, n_blocks))
            m64, b64 = sm.packed_words(n_blocks)
            _same(_raw(rekey_packed_host(key, m64, b64, n_blocks)), sm.rekey_packed(spec, m64, b64, n_blocks, tally=total),
                  ("packed", name, n_blocks))
        for n_chars in sm.WINDOW_CHARS:
            c = _compact(n_chars)
            for first, count in sm.windows(n_chars):
                got = store_packed_host(key, c, first, count)
                want = sm.store_packed(spec, c.mask32, c.body32, 4 * n_chars, first, count, tally=total)
                assert got.first_coef == want[2]
                _same(_raw(got), want[:2], ("window", name, n_chars, first, count))
    _all_reached(total, "monomial re-key keys, all runs")


# ---- select ------------------------------------------------------------------------------------------------------------
def _indices(n_chars, row_chars):
    _, _, rot, levels = sm.geometry(n_chars, row_chars)
    return [i for i in range(1 << (rot + levels)) if sm.names_a_row_or_a_missing_node(n_chars, row_chars, i)]


def test_gadget_queries_return_the_source_row():
    from fhestring_amd.api import select_bits, select_host
    pairs = 0
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        for n_chars, row_chars in sm.SHAPES:
            groups, row_blocks, rot, levels = sm.geometry(n_chars, row_chars)
            bits = rot + levels
            assert bits == select_bits(n_chars, row_chars)
            mask, body = sm.entry_words(n_chars)
            idx = _indices(n_chars, row_chars)
            rows = n_chars // row_chars
            missing = [i for i in idx if i >= rows]
            assert idx[:rows] == list(range(rows)) and all((i >> rot) >= groups for i in missing)
            got = list(pool.map(lambda i: select_host(sm.query(sm.gadget_query(i, bits)), mask, body, 4 * n_chars, row_chars), idx))
            for i, g in zip(idx, got):
                want = sm.selected_row(mask, body, n_chars, row_chars, i)
                assert i < rows or not (want[0].any() or want[1].any())
                _same(g, want, ("gadget query", n_chars, row_chars, i))
            pairs += len(idx)
            print("gadget queries, %d x %d characters: %d rows and %d missing nodes" % (rows, row_chars, rows, len(missing)))
    assert pairs == 2 + 512 + 2 + (3 + 1) + 5 + (41 + 16)


def test_monomial_queries_equal_the_model():
    from fhestring_amd.api import select_host
    total = sm.Tally()
    words = set()
    for n_chars, row_chars in sm.MONOMIAL_SHAPES:
        _, _, rot, levels = sm.geometry(n_chars, row_chars)
        mask, body = sm.entry_words(n_chars)
        for name, spec in sm.select_specs(rot + levels).items():
            assert rot + levels == 1 or any(rows == sm.gadget_bit(1) for rows in spec)
            words |= {w for rows in spec for row in rows for w, _ in row}
            want = sm.select(spec, mask, body, n_chars, row_chars, tally=total)
            _same(select_host(sm.query(spec), mask, body, 4 * n_chars, row_chars), want, ("monomial query", name, n_chars, row_chars))
            assert want[0].any() and want[1].any()
    assert words >= set(sm.KEY_WORDS)
    _all_reached(total, "monomial queries, all runs")


def test_select_host_equals_schoolbook_off_one_shape():
    """test_select.py holds the host reference against the schoolbook product at (1536, 256) alone"""
    from fhestring_amd.api import MyClientKey, select_host
    from test_select import _np_select
    client = MyClientKey(0xA11CE)
    rng = np.random.default_rng(29)
    try:
        for n_chars, row_chars, indices in ((512, 1, (0, 341)), (2624, 64, (13, 40))):
            groups = sm.geometry(n_chars, row_chars)[0]
            mask = rng.integers(0, 1 << 32, (groups, N), dtype=np.uint32)
            body = rng.integers(0, 1 << 32, 4 * n_chars, dtype=np.uint32)
            for index in indices:
                query = client.select_query(index, n_chars, row_chars)[0]
                _same(select_host(query, mask, body, 4 * n_chars, row_chars), _np_select(query, mask, body, n_chars, row_chars),
                      ("schoolbook", n_chars, row_chars, index))
    finally:
        client.close()


# ---- dense keys and the top of the exact range -------------------------------------------------------------------------------
def _magnitude(digs, polys, what, at_least):
    top = max(abs(sm.true_sum(digs, polys, n)) for n in (0, N // 2, N - 1))
    print("%s: largest true keyswitch sum 2^%.2f grid units (CRT range 2^93.0)" % (what, math.log2(top)))
    assert top >= at_least and top < 1 << 93
    return top


def _dense_rekey(key, n_blocks, mask, body, m64, b64, what):
    from fhestring_amd.api import CompactFheString, rekey_host, rekey_packed_host, store_packed_host
    _same(rekey_host(key, mask, body, n_blocks), sm.rekey(key, mask, body, n_blocks), (what, "re-key"))
    _same(_raw(rekey_packed_host(key, m64, b64, n_blocks)), sm.rekey_packed(key, m64, b64, n_blocks), (what, "packed"))
    n_chars = n_blocks // 4
    first, count = n_chars // 2, n_chars - n_chars // 2
    got = store_packed_host(key, CompactFheString(n_chars, mask, body), first, count)
    _same(_raw(got), sm.store_packed(key, mask, body, n_blocks, first, count)[:2], (what, "window"))


def test_dense_extreme_keys_equal_the_schoolbook():
    from fhestring_amd.api import REKEY_KEY_WORDS, SELECT_QUERY_BIT_WORDS, select_host
    rng = np.random.default_rng(5)
    key = rng.choice(np.array(sm.pm.KEY_WORDS, U64), REKEY_KEY_WORDS)
    n_blocks = CONTROL_BLOCKS
    mask, body = sm.rekey_words(n_blocks)
    _dense_rekey(key, n_blocks, mask, body, *sm.packed_words(n_blocks), "dense key")
    _magnitude(sm.digits2(mask[0]), key.reshape(2, 2, N)[:, 0], "dense re-key key, chosen words", 1 << 70)
    for n_chars, row_chars in ((2, 1), (1536, 512)):         # one rotate; two tree levels with a null sibling
        _, _, rot, levels = sm.geometry(n_chars, row_chars)
        query = rng.choice(np.array(sm.pm.KEY_WORDS, U64), (rot + levels) * SELECT_QUERY_BIT_WORDS).reshape(-1, 4, 2, N)
        m, b = sm.entry_words(n_chars)
        _same(select_host(query, m, b, 4 * n_chars, row_chars), sm.select(query, m, b, n_chars, row_chars), ("dense query", n_chars, row_chars))


def test_every_digit_minus_2_15_under_the_largest_key():
    """every key coefficient the largest grid word, every digit -2^15: the largest true sum that the two-digit and the
    four-digit keyswitch can meet (DESIGN.md sections 14 and 23: 2^84 and 2^85 grid units)"""
    from fhestring_amd.api import REKEY_KEY_WORDS, SELECT_QUERY_BIT_WORDS, select_host
    n_blocks = N
    key = np.full(REKEY_KEY_WORDS, sm.EXTREME_KEY_WORD, U64)
    mask = np.full((1, N), sm.EXTREME_WORD, np.uint32)
    body = np.full(n_blocks, sm.EXTREME_WORD, np.uint32)
    digs = sm.digits2(mask[0])
    assert all((d == -(1 << 15)).all() for d in digs)
    m64, b64 = sm.packed_words(n_blocks)
    m64[:] = U64(sm.EXTREME_WORD) << U64(32)
    _dense_rekey(key, n_blocks, mask, body, m64, b64, "all -2^15")
    top = _magnitude(digs, key.reshape(2, 2, N)[:, 0], "re-key, every digit -2^15", (1 << 84) - (1 << 80))
    assert top == 2 * N * (1 << 15) * ((1 << 57) - 1)
    n_chars, row_chars = 1024, 512                           # one tree level, no rotate: a = group 0 = 0, b = group 1
    query = np.full(SELECT_QUERY_BIT_WORDS, sm.EXTREME_KEY_WORD, U64).reshape(1, 4, 2, N)
    m, b = np.zeros((2, N), np.uint32), np.zeros(2 * N, np.uint32)
    m[1], b[N:] = sm.EXTREME_WORD, sm.EXTREME_WORD
    _same(select_host(query, m, b, 4 * n_chars, row_chars), sm.select(query, m, b, n_chars, row_chars), ("all -2^15", "select"))
    top = _magnitude(digs + digs, query[0, :, 0], "select, every digit -2^15", (1 << 85) - (1 << 81))
    assert top == 4 * N * (1 << 15) * ((1 << 57) - 1)


# ---- negative controls -------------------------------------------------------------------------------------------------------
_FORMATS = ("re-key", "packed", "window")
_BIG = ((512, 1), (2624, 64))
_AB = [(k, s, None) for k in _FORMATS for s in (sm.A_KEY, sm.B_KEY)]
# Which cases a wrong formula must show in, (kind, key or query or index, shape), by this reasoning:
CONTROLS = {
    # a truncated store moves every word whose dropped bits reach half, a dropped low carry is 2^16 c, a top digit of
    # +2^15 is 2^16 c as well: visible under any key word c that is no multiple of 2^48, with the mask words that carry
    # (0x8000, 0x7FFF8000, 0xFFFFFFFF): all three formats, both boundary keys, both queries
    **{f: _AB + [("monomial", q, sh) for sh in _BIG for q in (sm.A_QUERY, sm.B_QUERY)]
       for f in ("stores_round", "low_carry_kept", "top_carry_dropped")},
    # a tie needs an odd digit times 2^31 (2^47) next to words that vanish below it: the boundary keys, and the query that
    # begins with 2^31
    "tie_rounds_up": _AB + [("monomial", sm.A_QUERY, sh) for sh in _BIG],
    # 32 d more or less shows where the sum stands on a tie: the two keys built for it, and 0x1F next to 2^31 in a query
    "key_on_grid": [("re-key", sm.OFF32_KEY, None), ("packed", sm.OFF16_KEY, None), ("window", sm.OFF16_KEY, None)] +
                   [("monomial", sm.A_QUERY, sh) for sh in _BIG],
    "packed_mask_rounds_in": [("packed", sm.A_KEY, None), ("packed", sm.B_KEY, None)],
    # a rotate shows in the mask's wrapped words under any set bit
    "rotate_wrap_negates": [("gadget", 1, (2, 1)), ("gadget", 5, (512, 1)), ("gadget", 13, (2624, 64)), ("monomial", sm.A_QUERY, (2, 1)),
                            ("monomial", sm.B_QUERY, (512, 1)), ("monomial", sm.A_QUERY, (2624, 64))],
    # index 3 of three groups and indices 48.. of six name a missing node: zeros, not the even child
    "dead_sibling_is_zero": [("gadget", 3, (1536, 512)), ("gadget", 56, (2624, 64)), ("monomial", sm.A_QUERY, (1536, 512)),
                             ("monomial", sm.B_QUERY, (2624, 64))],
    # r = 2 and r = 3: group 1 is index 4 and index 8 (at r = 0, 1536 x 512, both rules are one)
    "tree_bit_above_rotates": [("gadget", 4, (640, 128)), ("gadget", 8, (2624, 64)), ("monomial", sm.A_QUERY, (2624, 64)),
                               ("monomial", sm.B_QUERY, (2624, 64))],
    # a monomial X^e with e > 0 rolls the absent bodies' digits into the stored words; under the second query bit 4 of
    # 41 x 64 is a set gadget bit and drops the last group with its null sibling, so that case is the first query's alone
    "absent_body_is_zero": [("monomial", sm.A_QUERY, (640, 128)), ("monomial", sm.B_QUERY, (640, 128)), ("monomial", sm.A_QUERY, (2624, 64))],
}


@pytest.fixture(scope="module")
def case(specs):
    """(host reference, model as a function of the rules) per case, the reference computed once and left unchanged"""
    from fhestring_amd.api import rekey_host, rekey_packed_host, select_host, store_packed_host
    done = {}

    def get(kind, which, shape):
        if (kind, which, shape) in done:
            return done[kind, which, shape]
        if kind in _FORMATS:
            spec = specs[which]
            key = sm.rekey_key(spec)
            if kind == "re-key":
                mask, body = sm.rekey_words(CONTROL_BLOCKS)
                ref = rekey_host(key, mask, body, CONTROL_BLOCKS)
                model = lambda rules: sm.rekey(spec, mask, body, CONTROL_BLOCKS, rules)
            elif kind == "packed":
                m64, b64 = sm.packed_words(CONTROL_BLOCKS)
                ref = _raw(rekey_packed_host(key, m64, b64, CONTROL_BLOCKS))
                model = lambda rules: sm.rekey_packed(spec, m64, b64, CONTROL_BLOCKS, rules)
            else:
                c = _compact(CONTROL_CHARS)
                ref = _raw(store_packed_host(key, c, 0, CONTROL_CHARS))
                model = lambda rules: sm.store_packed(spec, c.mask32, c.body32, 4 * CONTROL_CHARS, 0, CONTROL_CHARS, rules)[:2]
        else:
            n_chars, row_chars = shape
            _, _, rot, levels = sm.geometry(n_chars, row_chars)
            spec = sm.gadget_query(which, rot + levels) if kind == "gadget" else sm.select_specs(rot + levels)[which]
            mask, body = sm.entry_words(n_chars)
            ref = select_host(sm.query(spec), mask, body, 4 * n_chars, row_chars)
            model = lambda rules: sm.select(spec, mask, body, n_chars, row_chars, rules)
        for a in ref:
            a.setflags(write=False)
        _same(ref, model(sm.RIGHT), ("the right model", kind, which, shape))
        done[kind, which, shape] = ref, model
        return done[kind, which, shape]
    return get


def test_every_rule_has_its_control():
    assert set(CONTROLS) == {f.name for f in dataclasses.fields(sm.Rules)}
    assert all(f.default is True for f in dataclasses.fields(sm.Rules))


@pytest.mark.parametrize("error", [f.name for f in dataclasses.fields(sm.Rules)])
def test_a_wrong_model_differs_from_the_reference(case, error):
    """negative control: with one formula wrong the model must miss the host reference (which the right model equals) in
    every case listed for it"""
    wrong = dataclasses.replace(sm.RIGHT, **{error: False})
    for kind, which, shape in CONTROLS[error]:
        ref, model = case(kind, which, shape)
        got = model(wrong)
        differ = sum(int((np.asarray(g).reshape(-1) != np.asarray(r).reshape(-1)).sum()) for g, r in zip(got, ref))
        print("%s wrong, %s, %s%s: %d words differ" % (error, kind, which, "" if shape is None else ", %d x %d" % shape, differ))
        assert differ > 0, (error, kind, which, shape)
