"""The integer references of tests/synth_key.py against the CPU oracle, and the conditions on the fixed row set that the
GPU tests (tests/test_gpu_synth_key.py) rely on: numpy == Goldilocks NTT == schoolbook == the exact two-bit algorithm
bit for bit, the row set reaches the exact decomposition ties (tie count, mutation check), and the f64 mirrors stay
within T3 / T4 of the integer references on one-product rows."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import synth_key as sk
from oracle import core, radix


@pytest.fixture(scope="module")
def mat():
    return sk.material()


@pytest.fixture(scope="module")
def ref():
    return sk.references()


@pytest.fixture(scope="module")
def osk(mat):
    # the blind-rotation entry never touches the keyswitch key
    return core.ServerKey(mat.bsk, np.zeros(core.KSK_WORDS, np.uint64)).set_mb2(mat.bsk_mb2)


def _oracle(osk, ms, luts, lut_idx, rows, mode):
    """orc_blind_rotate on the given rows -> {row: [2][2048]}, a few rows at a time (ctypes releases the GIL)."""
    with ThreadPoolExecutor(4) as pool:
        accs = pool.map(lambda r: osk.blind_rotate(ms[r], luts[lut_idx[r]], mode=mode).reshape(2, sk.N), rows)
        return dict(zip(rows, accs))


@pytest.fixture(scope="module")
def schoolbook(mat, osk):
    rows = sk.rows_of(mat, "single", "pair", "sparse", "zero")
    return _oracle(osk, mat.ms, mat.luts, mat.lut_idx, rows, 1)


def test_row_set_covers_what_it_claims(mat):
    R = len(mat.ks)
    assert R <= 80 and mat.ks.shape == (R, 743) and len(mat.lut_idx) == R
    assert np.array_equal(mat.luts[3], radix.lut_poly("msg"))
    assert np.all(mat.luts[2] == np.uint64(1 << 62))
    low = mat.luts[:2] & np.uint64((1 << 41) - 1)
    assert set(np.unique(low).tolist()) == set(sk.EDGE_LOW)
    for kind, n in (("single", 18), ("pair", 8), ("sparse", 40), ("full", 4), ("zero", 2)):
        assert len(sk.rows_of(mat, kind)) == n
    nz = (mat.ms[:, :742] != 0).sum(axis=1)
    assert all(nz[r] == 1 for r in sk.rows_of(mat, "single")) and all(nz[r] == 24 for r in sk.rows_of(mat, "sparse"))
    assert all(nz[r] == 0 for r in sk.rows_of(mat, "zero")) and all(nz[r] >= 700 for r in sk.rows_of(mat, "full"))
    pairs = (mat.ms[:, 0:742:2] | mat.ms[:, 1:742:2]) != 0
    assert all(pairs[r].sum() == 1 for r in sk.rows_of(mat, "single", "pair"))
    got = {(int(mat.ms[r, 2 * p]), int(mat.ms[r, 2 * p + 1])) for r in sk.rows_of(mat, "pair") for p in np.flatnonzero(pairs[r])}
    assert got == set(sk.PAIR_SHAPES)
    # mask elements: every exponent with key bit 0 and with key bit 1 on the sparse rows; on the one-product rows every
    # exponent once, and 2048 with both key bits
    def seen(kind):
        return {(int(mat.ms[r, i]), int(mat.s[i])) for r in sk.rows_of(mat, kind) for i in np.flatnonzero(mat.ms[r, :742])}
    assert {(e, b) for e in sk.EXPONENTS for b in (0, 1)} <= seen("sparse")
    assert set(sk.EXPONENTS) <= {e for e, _ in seen("single")}
    assert {(2048, 0), (2048, 1)} <= seen("single")
    # bodies: every exponent
    assert set(sk.EXPONENTS) <= {int(b) for b in mat.ms[:, 742]}
    # modulus-switch edges: words that are not a << 52, in mask elements and in bodies
    ks = mat.ks
    frac = ks & np.uint64((1 << 52) - 1)
    for col in (slice(0, 742), slice(742, 743)):
        assert np.any(frac[:, col] == np.uint64((1 << 51) - 1)) and np.any(frac[:, col] == np.uint64(1 << 51))
        assert np.any(ks[:, col] == np.uint64(0xFFF8000000000000))
    assert np.any(ks[:, 742] == np.uint64(0xFFF7FFFFFFFFFFFF)) and np.any(ks[:, :742] == np.uint64(0xFFF7FFFFFFFFFFFF))
    assert np.all(mat.ms[ks == np.uint64(0xFFF8000000000000)] == 0) and np.all(mat.ms[ks == np.uint64(0xFFF7FFFFFFFFFFFF)] == 4095)
    assert np.array_equal(sk.mod_switch(np.array([(5 << 52) + (1 << 51) - 1, (5 << 52) + (1 << 51)], np.uint64)), [5, 6])


def test_every_key_word_is_a_multiple_of_2_pow_41(mat):
    for key, n in ((mat.bsk, 742), (mat.bsk_mb2, 1113)):
        assert key.shape == (n, 2, 2, 2048)
        assert not np.any(key & np.uint64((1 << 41) - 1))
        assert np.all((key != 0).sum(axis=3) >= 1) and np.all((key != 0).sum(axis=3) <= 2)
    s = mat.s
    assert np.array_equal(sk.pair_bits(s).reshape(371, 3),
                          np.stack([s[0::2] & (1 - s[1::2]), (1 - s[0::2]) & s[1::2], s[0::2] & s[1::2]], axis=1))


def test_classic_reference_equals_the_ntt_oracle_on_every_row(mat, ref, osk):
    got = _oracle(osk, mat.ms, mat.luts, mat.lut_idx, list(range(len(mat.ks))), 0)
    assert [r for r, acc in got.items() if not np.array_equal(acc, ref.acc[r])] == []


def test_classic_reference_equals_schoolbook(mat, ref, schoolbook):
    assert len(schoolbook) == 68
    assert [r for r, acc in schoolbook.items() if not np.array_equal(acc, ref.acc[r])] == []


def test_two_bit_reference_equals_the_exact_two_bit_oracle_on_every_row(mat, ref, osk):
    got = _oracle(osk, mat.ms, mat.luts, mat.lut_idx, list(range(len(mat.ks))), 5)
    assert [r for r, acc in got.items() if not np.array_equal(acc, ref.acc_mb2[r])] == []


def test_exact_ties_occur_in_the_products_of_the_row_set(mat, ref):
    n_products = int((mat.ms[:, :742] != 0).sum())
    assert len(ref.ties) == n_products
    mean = sum(ref.ties) / n_products
    print("exact ties per product: mean %.1f over %d products" % (mean, n_products))
    assert mean >= sk.MIN_TIES_PER_PRODUCT


def test_a_reference_that_rounds_ties_down_is_caught_on_the_edge_lut_rows(mat, ref, schoolbook):
    """Mutation check of the reference: with digit() adding 2^40 - 1 the comparison with schoolbook fails on every row
    with an edge LUT and a product -- the row set reaches the ties -- and on no other row (only ties changed).  The
    exception are rows that rotate by X^2048 only: the difference is -2 ACC, whose low 41 bits are even multiples of the
    edge values, never 2^40."""
    for r, want in schoolbook.items():
        lut = mat.lut_idx[r]
        mutant = sk.blind_rotate_ref(mat.desc, mat.ms[r], mat.luts[lut], digit=sk.digit_ties_down)
        reaches = lut < 2 and mat.kinds[r] != "zero" and np.any(mat.ms[r, :742] % 2048)
        assert np.array_equal(mutant, want) != reaches, (r, mat.kinds[r], int(lut))
    r = sk.rows_of(mat, "pair")[0]
    mutant = sk.blind_rotate_mb2_ref(mat.desc_mb2, mat.ms[r], mat.luts[mat.lut_idx[r]], digit=sk.digit_ties_down)
    assert not np.array_equal(mutant, ref.acc_mb2[r])


def test_f64_mirrors_stay_within_their_bounds_on_one_product_rows(mat, ref, osk):
    """Oracle mode 3 against the classic reference on the single-product rows, mode 4 against the two-bit reference on
    the single-pair rows: the digits are integers before the transform, the difference is the f64 rounding of one
    product.  T3 and T4 (synth_key.py) are 8 x the maxima measured here; the mirrors are bit-identical to the kernels."""
    single, one_pair = sk.rows_of(mat, "single"), sk.rows_of(mat, "single", "pair")
    m3 = _oracle(osk, mat.ms, mat.luts, mat.lut_idx, single, 3)
    m4 = _oracle(osk, mat.ms, mat.luts, mat.lut_idx, one_pair, 4)
    d3 = max(sk.centred_abs_max(m3[r], ref.acc[r]) for r in single)
    d4 = max(sk.centred_abs_max(m4[r], ref.acc_mb2[r]) for r in one_pair)
    print("max |mode 3 - reference| = 2^%.2f, max |mode 4 - reference| = 2^%.2f" % (math.log2(max(d3, 1)), math.log2(max(d4, 1))))
    assert d3 < sk.T3 and d4 < sk.T4
    assert sk.T3 < 2.0 ** 30 and sk.T4 < 2.0 ** 30          # 2^11 below one digit step of 2^41


def test_full_rows_rotate_the_lut_by_the_phase(mat, ref):
    """Sanity of the construction: the keys are GGSWs of the bits under S = X^js, so B - S * A of a full row is
    X^(sum a_i s_i - b) * lut up to the decomposition's rounding, below 2^52 in every coefficient."""
    worst = 0
    for r in sk.rows_of(mat, "full"):
        ms = mat.ms[r].astype(np.int64)
        e = int((ms[:742] * mat.s).sum() - ms[742]) % 4096
        for acc in (ref.acc[r], ref.acc_mb2[r]):
            worst = max(worst, sk.centred_abs_max(acc[1] - sk.rot(acc[0], mat.js), sk.rot(mat.luts[mat.lut_idx[r]], e)))
    print("max phase error of a full row = 2^%.2f" % math.log2(worst))
    assert worst < 1 << 52


def test_ntt_oracle_equals_schoolbook_on_the_chosen_masks_under_the_dense_key(mat, oracle_sk):
    """The rows of tests/test_gpu_synth_key.py's dense-key item: exact ties in the first product under a real key."""
    ks, ms, lut_idx = sk.dense_case()
    rows = list(range(len(ms)))
    m0 = _oracle(oracle_sk, ms, mat.luts, lut_idx, rows, 0)
    m1 = _oracle(oracle_sk, ms, mat.luts, lut_idx, rows, 1)
    assert [r for r in rows if not np.array_equal(m0[r], m1[r])] == []
