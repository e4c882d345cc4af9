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


# ---- keyswitch under the synthetic key -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kmat():
    return sk.keyswitch_material()


@pytest.fixture(scope="module")
def kref():
    return sk.keyswitch_reference()


@pytest.fixture(scope="module")
def krounding(kmat):
    """The mod-switched reference with the 15-bit input rounding adding 2^48 - 1 and 2^48 + 1 instead of 2^48."""
    return [sk.mod_switch(sk.keyswitch_ref(kmat.ksk, kmat.cts, r)) for r in ((1 << 48) - 1, (1 << 48) + 1)]


@pytest.fixture(scope="module")
def kdigits(kmat):
    return sk.ks_digits(kmat.cts[:, :2048]).view(np.uint64)


def _tile_positions(rows, width=128):
    """Positions inside a tile of 32 at which the given distinct rows appear in a batch of `width`."""
    src = sk.ks_batch(width)
    return {int(b) % 32 for b in np.flatnonzero(np.isin(src, list(rows)))}


def test_keyswitch_reference_equals_the_oracle_in_all_64_bits(kmat, kref):
    osk = core.ServerKey(np.zeros(core.BSK_WORDS, np.uint64), kmat.ksk)
    with ThreadPoolExecutor(4) as pool:
        raw = list(pool.map(osk.keyswitch, kmat.cts))
        switched = list(pool.map(osk.keyswitch_modswitch, kmat.cts))
    assert [r for r in range(sk.KS_ROWS) if not np.array_equal(raw[r], kref[r])] == []
    assert [r for r in range(sk.KS_ROWS) if not np.array_equal(switched[r], sk.mod_switch(kref[r]))] == []


def test_keyswitch_key_and_rows_are_what_they_claim(kmat, kref, krounding):
    U = np.uint64
    assert kmat.ksk.shape == (10240, 743) and kmat.cts.shape == (sk.KS_ROWS, 2049) and sk.KS_ROWS <= 64
    assert math.gcd(sk.KS_ROWS, 32) == 1 and len({c.tobytes() for c in kmat.cts}) == sk.KS_ROWS
    for kind, n in (("edge", 28), ("input", 28), ("full", 4), ("neg4", 1), ("pos3", 1), ("zero", 1)):
        assert kmat.kinds.count(kind) == n
    assert {w: sk.ks_launch_shape(w) for w in sk.KS_WIDTHS} == sk.KS_SHAPES_256
    # the key.  Top part: one coefficient per column, -2^(61 - 3 l), nothing else in those rows
    key = kmat.ksk.reshape(2048, 5, 743)
    assert len(set(kmat.top.tolist()) | set(kmat.dense.tolist())) == 2048 and len(kmat.top) == 742
    top = key[kmat.top]
    for l in range(5):
        assert np.all(top[np.arange(742), l, np.arange(742)] == U((1 << 64) - (1 << (61 - 3 * l))))
    assert np.count_nonzero(top) == 742 * 5
    # dense part: full words in every column; four levels equal, the twin one more; -128 and 127 in every byte plane of
    # every column tile; the words whose carry runs through all planes in every column
    dense = key[kmat.dense]
    twin = dense[np.arange(len(kmat.dense)), kmat.twin]
    for l in range(5):
        assert np.all(dense[:, l] + (kmat.twin != l).astype(U)[:, None] == twin)
    planes = sk.balanced_bytes(dense[:, 0])                       # [1306][743][8]
    for tile in range(24):
        p = planes[:, 32 * tile:32 * tile + 32]
        assert np.all(p.min(axis=(0, 1)) == -128) and np.all(p.max(axis=(0, 1)) == 127), tile
    for w in sk.KS_SPECIAL[16:]:
        assert np.all((dense[:, 0] == U(w)).any(axis=0)), hex(w)
    assert np.array_equal(sk.balanced_bytes(np.array([0x8080808080808080, 0x7F7F7F7F7F7F7F7F, (1 << 64) - 1, 0x80], U)),
                          [[-128, -127, -127, -127, -127, -127, -127, -127], [127] * 8, [-1, 0, 0, 0, 0, 0, 0, 0],
                           [-128, 1, 0, 0, 0, 0, 0, 0]])
    # every key word that exists meets a non-zero digit on an edge row of residual 0 and on one of residual -1
    d = sk.ks_digits(kmat.cts[:, :2048])
    for res in (0, -1):
        rows = [r for r, x in kmat.residual.items() if x == res]
        assert len(rows) >= 9 and np.all((d[rows] != 0).any(axis=0)), res
    assert {1, 0, -1} == set(kmat.residual.values())
    # edge rows: every one of the 743 outputs is edge + residual; input rows: three quarters of them
    for r, res in kmat.residual.items():
        on_edge = ((kref[r] - U(res & ((1 << 64) - 1))) & U((1 << 52) - 1)) == U(1 << 51)
        assert on_edge[742] and (on_edge.all() if kmat.kinds[r] == "edge" else on_edge.sum() >= 550), r
    # input-side edges, each in a tile's first and last row of a batch of 128 (and so of every wider one)
    a = kmat.cts[:, :2048]
    low = a & U((1 << 49) - 1)
    want = sk.mod_switch(kref)
    ties_down, ties_up = (x[:, :742] for x in krounding)
    features = {
        "low 49 bits 2^48, the rounding decides an output": [r for r in range(sk.KS_ROWS) if np.any(
            (low[r, kmat.top] == U(1 << 48)) & (ties_down[r] != want[r, :742]))],
        "low 49 bits 2^48 - 1, the rounding decides an output": [r for r in range(sk.KS_ROWS) if np.any(
            (low[r, kmat.top] == U((1 << 48) - 1)) & (ties_up[r] != want[r, :742]))],
        "wraps to zero": [r for r in range(sk.KS_ROWS) if np.any(a[r] >= U((1 << 64) - (1 << 48)))],
        "the first and the last word that wrap": [r for r in range(sk.KS_ROWS) if np.any(a[r] == U((1 << 64) - (1 << 48)))
                                                  and np.any(a[r] == U((1 << 64) - 1))],
        "every digit -4": [r for r in range(sk.KS_ROWS) if np.all(d[r] == -4)],
        "every digit 3": [r for r in range(sk.KS_ROWS) if np.all(d[r] == 3)],
        "zero mask": [r for r in range(sk.KS_ROWS) if not a[r].any()],
    }
    for name, rows in features.items():
        assert rows and {0, 31} <= _tile_positions(rows), (name, rows)
    wrapped = sk.ks_digits(np.array([[(1 << 64) - (1 << 48), (1 << 64) - 1, (1 << 64) - (1 << 48) - 1] + [0] * 2045], U))[0]
    assert not wrapped[:10].any() and list(wrapped[10:15]) == [0, 0, 0, 0, -1]


def test_a_wrong_byte_plane_is_caught_in_every_column_tile(kmat, kref, kdigits):
    """Mutation check of the row set, per byte plane b: the reference with ONE key word of a dense coefficient changed
    by +2^(8 b), and by -2^(8 b), changes a mod-switched output, for a word in each of the 24 column tiles -- for b = 0 a
    change of one unit in 64 bits.  Recomputing the same column with the unchanged key changes nothing."""
    U = np.uint64
    rng = np.random.default_rng(8)
    want = sk.mod_switch(kref)
    for b in range(8):
        for tile in range(24):
            j = 32 * tile + int(rng.integers(0, 32 if tile < 23 else 7))
            k = 5 * int(rng.choice(kmat.dense)) + int(rng.integers(0, 5))
            col = kmat.ksk[:, j:j + 1].copy()
            for sign in (1, -1):
                mutant = col.copy()
                mutant[k] += np.array([(sign << (8 * b)) & ((1 << 64) - 1)], U)
                got = _switch_column(mutant, kdigits, kmat.cts, j)
                assert np.any(got != want[:, j]), (b, tile, j, k, sign)
            assert np.array_equal(_switch_column(col, kdigits, kmat.cts, j), want[:, j]), (b, tile)
    # ... and a word of the top part, in the plane that holds it and in plane 0
    for j in (0, 741):
        for b in (0, 7):
            col = kmat.ksk[:, j:j + 1].copy()
            col[5 * int(kmat.top[j]) + 4] += np.array([1 << (8 * b)], U)
            assert np.any(_switch_column(col, kdigits, kmat.cts, j) != want[:, j]), (j, b)


def _switch_column(col, digits, cts, j):
    """Column j of the reference, mod-switched, from a key that holds this one column [10240][1]."""
    ks = np.uint64(0) - digits @ col[:, 0]
    return sk.mod_switch(ks + (cts[:, 2048] if j == 742 else np.uint64(0)))


def test_a_wrong_input_rounding_is_caught(kmat, kref, krounding):
    """Adding 2^48 - 1 instead of 2^48 (exact ties round down) changes mod-switched outputs on every edge and input row,
    and so does 2^48 + 1 on every input row."""
    want = sk.mod_switch(kref)
    down, up = krounding
    for r in kmat.residual:
        assert np.any(down[r] != want[r]), r
        assert kmat.kinds[r] != "input" or np.any(up[r] != want[r]), r


# ---- the exact arithmetics near the top of their CRT range -----------------------------------------------------------

@pytest.fixture(scope="module")
def xmat():
    return sk.extreme_material()


@pytest.fixture(scope="module")
def xref():
    return sk.extreme_references()


@pytest.fixture(scope="module")
def xosk(xmat):
    return core.ServerKey(xmat.bsk, np.zeros(core.KSK_WORDS, np.uint64)).set_mb2(xmat.bsk_mb2)


def test_extreme_keys_and_rows_are_what_they_claim(mat, xmat):
    U = np.uint64
    full = {1 << 63, (1 << 63) - (1 << 7)}
    dense = [(xmat.bsk, g) for g in sk.X_DENSE] + [(xmat.bsk_mb2, 3 * p + t) for p in sk.X_PAIRS for t in range(3)]
    for key, g in dense:
        assert set(np.unique(key[g]).tolist()) <= full
    assert np.all(xmat.bsk[400] == U(1 << 63)) and np.all(xmat.bsk_mb2[600:602] == U(1 << 63))
    # every other GGSW is the monomial one of material(), but for the mask polynomial of the two first steps
    same = np.ones(742, bool); same[list(sk.X_DENSE) + [sk.X_FIRST]] = False
    assert np.array_equal(xmat.bsk[same], mat.bsk[same])
    same = np.ones(1113, bool); same[[g for _, g in dense[3:]] + [3 * sk.X_FIRST_PAIR]] = False
    assert np.array_equal(xmat.bsk_mb2[same], mat.bsk_mb2[same])
    for key, g in ((xmat.bsk, sk.X_FIRST), (xmat.bsk_mb2, 3 * sk.X_FIRST_PAIR)):
        c = key[g, 1, 0][key[g, 1, 0] != 0]
        assert len(c) == 1 and int(c[0]) % (1 << 41) == 1 << 40
    assert not np.any(xmat.bsk & U(127)) and not np.any(xmat.bsk_mb2 & U(127))      # on both key grids
    assert np.all(xmat.luts[0] == U(1 << 62)) and np.all(xmat.luts[1] == U(1 << 63))
    assert len(xmat.ks) <= 40 and {"one", "pair", "two"} == set(xmat.kinds)
    assert 2048 in xmat.ms[:, :742] and np.all(xmat.ms[:, 742] == 0)
    assert {int(v) for v in xmat.ks[:, 742]} == {0, 0xFFF8000000000000, (1 << 51) - 1}


def test_extreme_references_equal_the_exact_oracles_in_every_word(xmat, xref, xosk):
    rows = list(range(len(xmat.ks)))
    for mode, want in ((1, xref.acc), (0, xref.acc), (5, xref.acc_mb2)):
        got = _oracle(xosk, xmat.ms, xmat.luts, xmat.lut_idx, rows, mode)
        assert [r for r in rows if not np.array_equal(got[r], want[r])] == [], mode


def test_extreme_rows_reach_the_top_of_the_crt_range(xmat, xref):
    """The largest coefficient of a dense product as a true integer in units of the key grid: the classic kernel is
    documented for |x| <= 2^91, the two-bit one for 2^92.6, the CRT range is p0 p1 / 2 = 2^93.0.  The range mutant --
    the true integers wrapped into (-M/2, M/2], then taken mod 2^64 -- equals the reference for M = p0 p1 (the products
    are inside the range) and differs for M = p0 p1 / 8 (classic) and p0 p1 / 4 (two-bit): the rows are where it matters."""
    M = sk.NTT_P0 * sk.NTT_P1
    assert 2 ** 92.99 < M // 2 < 2 ** 93
    for name, products, grid, need, shrink in (("classic", xref.products, 6, 90, 8), ("two-bit", xref.products_mb2, 7, 91, 4)):
        mags = [sk.true_magnitude(p) for p in products]
        by_kind = {k: max(m for m, kind in zip(mags, xmat.kinds) if kind == k) for k in ("one", "pair", "two")}
        print("%s: largest product coefficient 2^%.2f on one-step rows, 2^%.2f on one-pair rows, 2^%.2f on two-step rows"
              % (name, by_kind["one"], by_kind["pair"], by_kind["two"]))
        assert max(by_kind["one"], by_kind["pair"]) >= need, name             # the condition set for the one-step rows
        assert by_kind["two"] >= need + 1, name                               # both GGSW rows carry extreme digits
        assert max(mags) < math.log2(M // 2)
        differs = 0
        for found in products:
            for x_true, wrapping in found:
                assert np.array_equal(sk.wrap_to_range(x_true, M, grid), wrapping)
                differs += not np.array_equal(sk.wrap_to_range(x_true, M // shrink, grid), wrapping)
        assert differs >= 2, name


def test_f64_mirrors_stay_within_their_bounds_on_the_extreme_rows(xmat, xref, xosk):
    """Oracle modes 3 and 4 against the integer references at this magnitude, on the rows whose last step is their one dense
    product (a monomial first step adds 2^20 at most and leaves the digits of the dense step alone).  T3X and T4X (synth_key.py)
    are 8 x the maxima measured here.  They are ABOVE one digit step of 2^41: on a row with a step after a dense product that
    product's rounding changes the digits of the next, and the distance is whatever those digits make of the key (printed,
    not bounded) -- the kernels are held to their mirrors bit for bit on every row all the same."""
    rows = list(range(len(xmat.ks)))
    m3 = _oracle(xosk, xmat.ms, xmat.luts, xmat.lut_idx, rows, 3)
    m4 = _oracle(xosk, xmat.ms, xmat.luts, xmat.lut_idx, rows, 4)
    assert len(xmat.one_dense) >= 10 and xmat.one_dense_mb2 == rows
    d3 = max(sk.centred_abs_max(m3[r], xref.acc[r]) for r in xmat.one_dense)
    d4 = max(sk.centred_abs_max(m4[r], xref.acc_mb2[r]) for r in xmat.one_dense_mb2)
    rest = max(sk.centred_abs_max(m3[r], xref.acc[r]) for r in rows if r not in xmat.one_dense)
    print("extreme rows: max |mode 3 - reference| = 2^%.2f, max |mode 4 - reference| = 2^%.2f; mode 3 on rows with a "
          "step after a dense product 2^%.2f" % (math.log2(max(d3, 1)), math.log2(max(d4, 1)), math.log2(max(rest, 1))))
    assert d3 < sk.T3X and d4 < sk.T4X
    assert 2.0 ** 41 < sk.T3X < 2.0 ** 52 and 2.0 ** 41 < sk.T4X < 2.0 ** 52      # above a digit step, below a mod-switch step
