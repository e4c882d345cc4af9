"""The host reference of the packing tree (fhs_pack_host, fhs_debug_pack_node, fhs_pack_switch16) under synthetic keys
and on chosen words, against tests/pack_model.py: integer numpy with no product through a transform and no call into
the library.  Every comparison is exact word equality.

    zero key       every keyswitch sum vanishes: the packed GLWE has a closed form (the gather of the whole tree: the
                   monomial shift of every block, the leaf built from a block, the body doubled at every level)
    monomial keys  every key polynomial is one word times X^m: the tree is a recursion on 2048-vectors, node by node,
                   with the kernel's liveness rule (null siblings, trivial leaves)
    dense keys     one node per level against the schoolbook product, key words from the extremes of the grid rounding
    controls       the model with ONE formula wrong differs from the reference on these inputs: the inputs are sensitive

Half of all block words come from pack_model.BLOCK_WORDS (the prescale's rounding and wrap, 0, 2^63, 2^63 - 1, prescaled
values on the digit boundaries); how often a run reaches each boundary is counted by the model and printed (pytest -s).
tests/test_pack_synth_device.py runs the same inputs through the kernels."""
import dataclasses
import time

import numpy as np
import pytest

import pack_model as pm
from ring_util import round16

N = 2048
U64 = np.uint64
ZERO_KEY_COUNTS = (1, 4, 5, 12, 2048, 2052, 8196)
MONOMIAL_COUNTS = (1, 5, 12, 24, 300, 2052)
CONTROL_COUNTS = (5, 12)                                    # (one block has no odd child anywhere: nothing is shifted)


def _trivial(n):
    return [k for k in range(n) if k % 7 == 3]


@pytest.fixture(scope="module")
def specs():
    return pm.monomial_specs()


@pytest.fixture(scope="module")
def reference(specs):
    """pack_host under a monomial key, once per (key, block count): shared with the controls and left unchanged"""
    from fhestring_amd.api import pack_host
    done = {}

    def get(name, n):
        if (name, n) not in done:
            blocks = pm.chosen_blocks(np.random.default_rng(1000 + n), n, _trivial(n))
            m64, b64 = pack_host(pm.monomial_key(specs[name]), blocks)
            for a in (blocks, m64, b64):
                a.setflags(write=False)
            done[name, n] = blocks, m64, b64
        return done[name, n]
    return get


def test_zero_key_equals_the_closed_form():
    from fhestring_amd.api import PACK_KEY_WORDS, pack_host
    key = np.zeros(PACK_KEY_WORDS, U64)
    tally = pm.Tally()
    for n in ZERO_KEY_COUNTS:
        blocks = pm.chosen_blocks(np.random.default_rng(n), n, _trivial(n))
        t0 = time.perf_counter()
        want = pm.zero_key_pack(blocks)
        t1 = time.perf_counter()
        got = pack_host(key, blocks)
        assert np.array_equal(got[0], want[0]), "mask, %d blocks" % n
        assert np.array_equal(got[1], want[1]), "body, %d blocks" % n      # the whole polynomial: 0 beyond the count
        last = (n - 1) % N + 1
        assert not want[1][-1, last:].any() and (n < 2 or want[1][-1, :last].any())
        tally.prescale_words(blocks)
        tally.add(pm.round_classes(np.stack(want), 48))
        print("zero key, %d blocks: closed form %.3f s, pack_host %.3f s" % (n, t1 - t0, time.perf_counter() - t1))
        if n == 12:                                            # ... and the closed form is what the recursion gives
            zero_spec = [[[(0, 0)] * 2] * pm.LEVELS] * pm.TREE_LEVELS
            again = pm.tree(zero_spec, blocks)
            assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    print("boundaries reached under the zero key, all runs (round16: of the packed words, as the device test rounds them):\n%s" % tally)
    assert all(hits > 0 for hits in tally.counts.values()), tally.counts


def test_monomial_keys_equal_the_recursion(specs, reference):
    total = pm.Tally()
    for name, spec in specs.items():
        words = [w for level in spec for digit in level for w, _ in digit]
        exps = {m for level in spec for digit in level for _, m in digit}
        assert {0, N - 1} <= exps and set(words) == set(pm.KEY_WORDS)
        total.add(pm.key_classes(words))
        for n in MONOMIAL_COUNTS:
            blocks, m64, b64 = reference(name, n)
            assert ((blocks[:, :N] == 0).all(axis=1)).sum() == len(_trivial(n))
            assert np.isin(blocks, pm.BLOCK_WORDS).mean() >= 0.5
            tally = pm.Tally()
            t0 = time.perf_counter()
            want = pm.tree(spec, blocks, tally=tally)
            dt = time.perf_counter() - t0
            assert np.array_equal(m64, want[0]), "mask, key with %s, %d blocks" % (name, n)
            assert np.array_equal(b64, want[1]), "body, key with %s, %d blocks" % (name, n)
            print("key with %s, %d blocks: model %.2f s" % (name, n, dt))
            total.add(tally.counts)
            # every block count reaches every boundary of the prescale and of the digits, the full carry chain included
            for cls, hits in tally.counts.items():
                if cls.startswith(("prescale", "digits")):
                    assert hits > 0, (name, n, cls)
    print("boundaries reached under the monomial keys, all runs:\n%s" % total)
    assert all(total.counts[c] > 0 for c in total.counts if c.startswith("key")), total.counts


def test_dense_extreme_keys_node_by_node():
    """every level, key words drawn from the extremes of the grid rounding, E and O from the three-digit boundary words:
    O = 0 at the odd levels (the digits are the chosen words up to sign), one constant mask word at every third"""
    import fhestring_amd
    L = fhestring_amd.lib()
    rng = np.random.default_rng(3)
    key = rng.choice(np.array(pm.KEY_WORDS, U64), (pm.TREE_LEVELS, pm.LEVELS, 2, N))
    flat = np.ascontiguousarray(key.reshape(-1))
    print("dense key:\n%s" % "\n".join("    %-72s %d" % kv for kv in pm.key_classes(flat).items()))
    tally = pm.Tally()
    for lv in range(1, pm.TREE_LEVELS + 1):
        e = rng.choice(pm.NODE_WORDS, (2, N))
        o = np.zeros((2, N), U64) if lv % 2 else rng.choice(pm.NODE_WORDS, (2, N))
        if lv % 3 == 0:
            e[0, :] = pm.NODE_WORDS[(lv // 3 + 2) % len(pm.NODE_WORDS)]
        tally.digit_words(pm.merge(lv, e, o, pm.RIGHT)[1])
        got = np.zeros((2, N), U64)
        assert L.fhs_debug_pack_node(flat.ctypes.data, lv, e.ctypes.data, o.ctypes.data, got.ctypes.data) == 0
        assert np.array_equal(got, pm.node_dense(flat, lv, e, o)), lv
    print("boundaries reached by the eleven nodes:\n%s" % tally)
    assert all(hits > 0 for hits in tally.counts.values()), tally.counts


def test_switch16_on_chosen_words():
    from fhestring_amd.api import pack_switch16
    chosen = np.array([0x00007FFFFFFFFFFF, 0x0000800000000000, 0xFFFF7FFFFFFFFFFF, 0xFFFF800000000000, 0, (1 << 64) - 1,
                       0x7FFF800000000000, 0x7FFF7FFFFFFFFFFF, 1 << 63], U64)
    assert list(round16(chosen)) == [0, 1, 0xFFFF, 0, 0, 0, 0x8000, 0x7FFF, 0x8000]      # 0xFFFF8000...: the wrap to 0
    rng = np.random.default_rng(16)
    for n_blocks in (4, 2048, 2052):
        g = (n_blocks + N - 1) // N
        m64, b64 = rng.choice(chosen, (g, N)), rng.choice(chosen, (g, N))
        m64[:, :len(chosen)] = chosen
        b64[:, :4] = chosen[:4]
        p = pack_switch16(m64, b64, n_blocks)
        assert np.array_equal(p.mask16, round16(m64)), n_blocks
        assert np.array_equal(p.body16, round16(b64).reshape(-1)[:n_blocks]), n_blocks
        first = (n_blocks - 1) // N * N                         # the last group's bodies start at 2048 g
        assert list(p.body16[first:first + 4]) == [0, 1, 0xFFFF, 0]
    m16, b16 = pack_switch16(m64[:1], b64[:1], 3)               # not whole characters: the raw arrays
    assert np.array_equal(m16, round16(m64[:1])) and np.array_equal(b16, round16(b64[0, :3]))


CONTROLS = {"no negation where the monomial shift wraps": "shift_wrap_negates",
            "no sign in the automorphism": "automorphism_signed",
            "floor instead of round in the prescale": "prescale_rounds",
            "no rounding add in the digits": "digits_round",
            "key not rounded to the grid": "key_on_grid",
            "a dead odd child read as the even one": "dead_odd_is_zero"}


@pytest.mark.parametrize("error", list(CONTROLS))
def test_a_wrong_model_differs_from_the_reference(specs, reference, error):
    """negative control: with one formula wrong the model must miss the host reference (which the right model equals,
    above) in mask and body, under both keys and at both block counts"""
    assert set(CONTROLS.values()) == {f.name for f in dataclasses.fields(pm.Rules)}
    wrong = dataclasses.replace(pm.RIGHT, **{CONTROLS[error]: False})
    for name, spec in specs.items():
        for n in CONTROL_COUNTS:
            blocks, m64, b64 = reference(name, n)
            got = pm.tree(spec, blocks, rules=wrong)
            assert not np.array_equal(got[0], m64), (error, name, n, "mask")
            assert not np.array_equal(got[1], b64), (error, name, n, "body")


def test_a_wrong_closed_form_input_differs_under_the_zero_key():
    """... and the two controls that need no key, on the zero key's inputs: the closed form of floor-prescaled blocks and
    the recursion without the shift's negation both miss the reference"""
    from fhestring_amd.api import PACK_KEY_WORDS, pack_host
    blocks = pm.chosen_blocks(np.random.default_rng(12), 12, _trivial(12))
    got = pack_host(np.zeros(PACK_KEY_WORDS, U64), blocks)
    zero_spec = [[[(0, 0)] * 2] * pm.LEVELS] * pm.TREE_LEVELS
    for field in ("prescale_rounds", "shift_wrap_negates", "dead_odd_is_zero"):
        bad = pm.tree(zero_spec, blocks, rules=dataclasses.replace(pm.RIGHT, **{field: False}))
        assert not np.array_equal(bad[0], got[0]), field
