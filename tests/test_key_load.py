"""Key load under keys that do not lie on the key grid (tests/synth_key.py: offgrid_material), on the CPU: the integer
references, which round the loaded words with round_grid, against the oracle, which rounds in its own code -- numpy ==
Goldilocks NTT == schoolbook on the 2^6 grid, the exact two-bit algorithm on the 2^7 grid taken from the original word;
the rows that meet only words that return keep the outputs of the on-grid key; the f64 mirrors (oracle modes 3 and 4,
what tests/test_key_load_device.py holds the kernels to bit for bit) stay within T3 / T4 and T3U / T4U of the integer
references; and the negative control: a reference whose rounding truncates, rounds ties down, rounds the pair key to 2^6
and then to 2^7, or uses the other grid is told from the right one, by the rows of the class that can tell it."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import synth_key as sk
from oracle import core

U = np.uint64


@pytest.fixture(scope="module")
def base():
    return sk.material()


@pytest.fixture(scope="module")
def mat():
    return sk.offgrid_material()


@pytest.fixture(scope="module")
def ref():
    return sk.offgrid_references()


@pytest.fixture(scope="module")
def osk(mat):
    # the oracle rounds the words itself (orc_bsk_quantize; the 2^7 grid in orc_server_key_set_mb2)
    return core.ServerKey(mat.bsk, np.zeros(core.KSK_WORDS, U)).set_mb2(mat.bsk_mb2)


def _oracle(osk, mat, rows, mode):
    with ThreadPoolExecutor(4) as pool:
        accs = pool.map(lambda r: osk.blind_rotate(mat.ms[r], mat.luts[mat.lut_idx[r]], mode=mode).reshape(2, sk.N), rows)
        return dict(zip(rows, accs))


def _classes(mat, pair_key):
    """-> (the loaded key, material()'s, [n] bool: GGSW of class M, of class U)"""
    key, on_grid = (mat.bsk_mb2, sk.material().bsk_mb2) if pair_key else (mat.bsk, sk.material().bsk)
    m, u = np.zeros(len(key), bool), np.zeros(len(key), bool)
    m[sk._triples(mat.m_pairs) if pair_key else list(mat.m_dense)] = True
    u[sk._triples(mat.u_pairs) if pair_key else list(mat.u_dense)] = True
    return key, on_grid, m, u


def test_round_grid_is_the_rule_of_the_header():
    """round_to_grid of host_ntt.h on the words that decide: ties go up, the sum wraps."""
    top = 1 << 64
    cases = {6: [(0, 0), (31, 0), (32, 64), (33, 64), (95, 64), (96, 128), (top - 32, 0), (top - 33, top - 64), (top - 1, 0),
                 ((1 << 63) - 32, 1 << 63), ((1 << 63) - 33, (1 << 63) - 64), ((5 << 41) - 32, 5 << 41)],
             7: [(0, 0), (63, 0), (64, 128), (32, 0), (96, 128), (191, 128), (192, 256), (top - 64, 0), (top - 65, top - 128),
                 ((1 << 63) - 33, 1 << 63), ((1 << 63) - 64, 1 << 63), ((1 << 63) - 65, (1 << 63) - 128)]}
    for bits, pairs in cases.items():
        got = sk.round_grid(np.array([w for w, _ in pairs], U), bits)
        assert [int(v) for v in got] == [want for _, want in pairs], bits
    # "6 then 7" against 7 at once: different exactly for low 7 bits in [32, 63]
    w = np.arange(256, dtype=U) + U(3 << 41)
    differs = sk.round_6_then_7(w, 7) != sk.round_grid(w, 7)
    assert np.array_equal(differs, ((w & U(127)) >= U(32)) & ((w & U(127)) <= U(63)))


def test_offgrid_keys_and_rows_are_what_they_claim(base, mat):
    n_base = len(base.ks)
    for pair_key in (False, True):
        key, on_grid, m, u = _classes(mat, pair_key)
        r = ~(m | u)
        delta = (key - on_grid).view(np.int64)
        # class R: every word, zero words included, carries one of the offsets and returns on both grids
        assert set(np.unique(delta[r]).tolist()) == set(sk.R_OFFSETS)
        assert np.array_equal(sk.round_grid(key[r], 6), on_grid[r]) and np.array_equal(sk.round_grid(key[r], 7), on_grid[r])
        assert np.any(key[r] == U((1 << 64) - 1)) and np.any(key[r] == U((1 << 64) - 32))
        assert (key[r] & U(63)).all()
        # class M: the offsets, and the planted words where material() has zero; those near 2^63 in GGSW row 0 only
        plants = sk.M_PLANTS_WRAP + sk.M_PLANTS_TOP
        planted = np.isin(key[m], np.array(plants, U))
        assert set(np.unique(delta[m][~planted]).tolist()) == set(sk.M_OFFSETS)
        assert not on_grid[m][planted].any()
        for w in plants:
            per_poly = (key[m] == U(w)).sum(axis=3)                       # [GGSW][row][col]
            assert np.all(per_poly[:, 0] >= 2) and np.all(per_poly[:, 1] == (0 if w in sk.M_PLANTS_TOP else 4)), hex(w)
        for bits in (6, 7):
            moved = (sk.round_grid(key[m], bits) - on_grid[m]).view(np.int64)
            # the rounded polynomial is dense with 0, +-2^6 and 2^7 (2^6 grid) / 0 and 2^7 (2^7 grid: -64 is a tie, up to 0)
            steps = {-64, 0, 64, 128, (1 << 63) - 64, -(1 << 63)} if bits == 6 else {0, 128, -(1 << 63)}
            assert set(np.unique(moved).tolist()) == steps, bits
        assert np.any(sk.round_grid(key[m], 6) != sk.round_grid(key[m], 7))
        assert np.any(sk.round_6_then_7(key[m], 7) != sk.round_grid(key[m], 7))
        # class U: off the grid in (nearly) every word
        assert ((key[u] & U(63)) != 0).mean() > 0.9 and int(m.sum()) >= 5 and int(u.sum()) >= 3
    assert len(mat.m_dense) == 7 and len(mat.u_dense) == 3 and len(mat.u_pairs) == 2
    assert set(mat.m_pairs) == {g // 2 for g in mat.m_dense} and not set(mat.m_pairs) & set(mat.u_pairs)
    # rows: material()'s, the full ones without the mask elements of the U GGSWs, and the thirteen rows of class U
    changed = [r for r in range(n_base) if not np.array_equal(mat.ks[r], base.ks[r])]
    assert changed == sk.rows_of(base, "full") and mat.kinds[:n_base] == base.kinds
    assert not mat.ms[:n_base, list(mat.blocked)].any()
    u_rows = list(range(n_base, len(mat.ks)))
    assert len(u_rows) == 13 and not np.delete(mat.ms[u_rows, :742], list(mat.blocked) + [mat.u_first], axis=1).any()
    assert mat.u_first < min(mat.blocked) and mat.u_first // 2 not in mat.m_pairs + mat.u_pairs
    assert len(mat.one_u) == 9 and mat.one_u_mb2 == u_rows
    two_step = [r for r in u_rows if mat.ms[r, mat.u_first]]
    assert len(two_step) == 4 and all(mat.lut_idx[r] >= 2 for r in two_step) and len(set(two_step) & set(mat.one_u)) == 3
    assert len(mat.one_m) == 3 and len(mat.one_m_mb2) >= 5
    assert {base.kinds[r] for r in mat.m_rows} == {"single", "pair", "sparse", "full"}
    assert len(mat.r_rows) >= 40 and len(mat.r_rows_mb2) >= 40
    assert len([r for r in mat.r_rows if base.kinds[r] == "single"]) == 15
    assert 4 * len(mat.ks) <= 1024                     # the wide-LDS variant of the 4-wavefront kernel on 256 CUs


def test_rows_of_class_r_keep_the_outputs_of_the_on_grid_key(mat, ref):
    on_grid = sk.references()
    assert [r for r in mat.r_rows if not np.array_equal(ref.acc[r], on_grid.acc[r])] == []
    for acc in (ref.acc_mb2_6, ref.acc_mb2_7):
        assert [r for r in mat.r_rows_mb2 if not np.array_equal(acc[r], on_grid.acc_mb2[r])] == []
    # ... and the rows of class M do not, on either grid; the two grids of the pair key differ from each other
    assert [r for r in mat.m_rows if np.array_equal(ref.acc[r], on_grid.acc[r])] == []
    for acc in (ref.acc_mb2_6, ref.acc_mb2_7):
        assert [r for r in mat.m_rows_mb2 if np.array_equal(acc[r], on_grid.acc_mb2[r])] == []
    assert [r for r in mat.m_rows_mb2 if np.array_equal(ref.acc_mb2_6[r], ref.acc_mb2_7[r])] == []


def test_classic_reference_equals_the_ntt_oracle_and_schoolbook(mat, ref, osk):
    rows = list(range(len(mat.ks)))
    got = _oracle(osk, mat, rows, 0)
    assert [r for r in rows if not np.array_equal(got[r], ref.acc[r])] == []
    light = [r for r in rows if mat.kinds[r] != "full"]
    got = _oracle(osk, mat, light, 1)
    assert [r for r in light if not np.array_equal(got[r], ref.acc[r])] == []


def test_two_bit_reference_on_the_2_pow_7_grid_equals_the_exact_two_bit_oracle(mat, ref, osk):
    rows = list(range(len(mat.ks)))
    got = _oracle(osk, mat, rows, 5)
    assert [r for r in rows if not np.array_equal(got[r], ref.acc_mb2_7[r])] == []


def test_f64_mirrors_stay_within_their_bounds_of_the_integer_references(base, mat, ref, osk):
    """Modes 3 and 4 (the outputs that tests/test_key_load_device.py compares the kernels with) against the integer
    references on the 2^6 grid.  One-product rows of class R and M: the existing T3 / T4.  One-product rows of class U:
    T3U / T4U (synth_key.py) are 8 x the maxima measured here, against the integer reference and nothing else.  The
    bound tells the grids apart: the reference of the pair key on the 2^7 grid is further than T4 from mode 4 on every
    one-product row of class M."""
    one_r = [r for r in mat.r_rows if base.kinds[r] == "single"]
    one_r_mb2 = [r for r in mat.r_rows_mb2 if base.kinds[r] in ("single", "pair")]
    m3 = _oracle(osk, mat, one_r + mat.one_m + mat.one_u, 3)
    m4 = _oracle(osk, mat, one_r_mb2 + mat.one_m_mb2 + mat.one_u_mb2, 4)
    d3 = {name: max(sk.centred_abs_max(m3[r], ref.acc[r]) for r in rows)
          for name, rows in (("R", one_r), ("M", mat.one_m), ("U", mat.one_u))}
    d4 = {name: max(sk.centred_abs_max(m4[r], ref.acc_mb2_6[r]) for r in rows)
          for name, rows in (("R", one_r_mb2), ("M", mat.one_m_mb2), ("U", mat.one_u_mb2))}
    for mode, d in ((3, d3), (4, d4)):
        print("max |mode %d - reference| on one-product rows: %s" % (
            mode, ", ".join("class %s 2^%.2f" % (k, math.log2(max(v, 1))) for k, v in d.items())))
    assert max(d3["R"], d3["M"]) < sk.T3 and max(d4["R"], d4["M"]) < sk.T4
    assert d3["U"] < sk.T3U and d4["U"] < sk.T4U
    assert 8 * d3["U"] >= sk.T3U / 2 ** 0.01 and 8 * d4["U"] >= sk.T4U / 2 ** 0.01       # the figures are the measured ones
    assert sk.T3U < 2.0 ** 52 and sk.T4U < 2.0 ** 52                                     # below a modulus-switch step
    assert all(sk.centred_abs_max(m4[r], ref.acc_mb2_7[r]) > sk.T4 for r in mat.one_m_mb2)


# what each mutant of round_grid does to the words of class R, per (key, grid): they return under the right rounding on
# both grids, so a mutant that only confuses the grids cannot show on them, and the 2^7 grid has its ties at +-64, which
# do not return on the 2^6 grid and so are of class M.  On class M every mutant shows on every key and grid.
SHOWS_ON_CLASS_R = {("truncation", False, 6): True, ("truncation", True, 6): True, ("truncation", True, 7): True,
                    ("ties down", False, 6): True, ("ties down", True, 6): True, ("ties down", True, 7): False,
                    ("6 then 7", True, 7): False,
                    ("wrong grid", False, 6): False, ("wrong grid", True, 6): False, ("wrong grid", True, 7): False}


@pytest.mark.parametrize("name", list(sk.ROUND_MUTANTS))
def test_a_wrong_rounding_at_key_load_is_caught(base, mat, ref, name):
    """Per mutant, key and grid: the reference whose key is rounded by the mutant differs from the right one on EVERY
    chosen row of class M -- the one-product rows and the two-product rows -- and on every chosen row of class R where
    the table above says so (and on none where it says not: those words need class M).  The same code with round_grid
    itself reproduces the references."""
    mutant = sk.ROUND_MUTANTS[name]
    cases = [(pair_key, bits) for (n, pair_key, bits) in SHOWS_ON_CLASS_R if n == name]
    assert cases
    for pair_key, bits in cases:
        want = (ref.acc_mb2_7 if bits == 7 else ref.acc_mb2_6) if pair_key else ref.acc
        r_rows, m_rows = (mat.r_rows_mb2, mat.m_rows_mb2) if pair_key else (mat.r_rows, mat.m_rows)
        few = lambda rows: [r for r in rows if base.kinds[r] in ("single", "pair")][:5]
        chosen_r, chosen_m = few(r_rows), few(m_rows)
        assert len(chosen_r) == 5 and len(chosen_m) == 5
        for r in chosen_r + chosen_m:
            assert np.array_equal(sk.offgrid_row(mat, r, pair_key, bits, every=True), want[r]), (pair_key, bits, r)
        for r in chosen_m:
            assert not np.array_equal(sk.offgrid_row(mat, r, pair_key, bits, mutant, every=True), want[r]), (pair_key, bits, r)
        shows = SHOWS_ON_CLASS_R[(name, pair_key, bits)]
        for r in chosen_r:
            got = sk.offgrid_row(mat, r, pair_key, bits, mutant, every=True)
            assert np.array_equal(got, want[r]) != shows, (pair_key, bits, r)


def test_every_offset_occurs_in_a_polynomial_that_a_row_multiplies_with(mat, ref):
    """An offset that only occurs where every row has zero digits would hide a failure: per key, class and offset (and
    planted word) there is a GGSW row with that offset that met non-zero digits.  The words near 2^63 sit in GGSW row 0,
    which the rows with one product do not multiply with; the rows with more do."""
    for pair_key, used in ((False, ref.used), (True, ref.used_mb2)):
        key, on_grid, m, u = _classes(mat, pair_key)
        met = np.zeros((len(key), 2), bool)
        met[tuple(np.array(sorted(used)).T)] = True
        delta = (key - on_grid).view(np.int64)
        for cls, offsets in ((~(m | u), sk.R_OFFSETS), (m, sk.M_OFFSETS)):
            for off in offsets:
                assert np.any((delta == off).any(axis=(2, 3)) & met & cls[:, None]), (pair_key, off)
        for w in sk.M_PLANTS_WRAP + sk.M_PLANTS_TOP + ((1 << 64) - 1, (1 << 64) - 32):
            cls = m if w in sk.M_PLANTS_TOP else np.ones(len(key), bool)
            assert np.any((key == U(w)).any(axis=(2, 3)) & met & cls[:, None]), (pair_key, hex(w))
        assert np.all(met[m]) and np.all(met[u])            # every GGSW row of class M and U
    # the second product of a two-product row is one that multiplies with row 0 of a class-M GGSW
    light = set()
    for r in mat.m_rows:
        if mat.kinds[r] == "pair":
            sk.offgrid_row(mat, r, False, 6, used=light)
    assert any(row == 0 and g in mat.m_dense for g, row in light)
