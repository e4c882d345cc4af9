"""The shifted accumulator of blind_rotate_fft_kernel (csrc/fft_kernels.hip, SHIFTED = true) against the general form,
as integer models in numpy (u64 / u32 with wrap-around), operation for operation:

  general   am = a - 1, vm = v - 1;  t = vm or ~vm (flipped), borrow-in 1 where NOT flipped
            nhi = hi32(am - t - borrow);  digit = (int32)(0xFF - nhi) >> 9;  am' = am + (b << 12)
  shifted   A = am >> 8, V = vm >> 8 with ANYTHING in the top 8 bits of either word; the same subtraction
            nhi = hi32(A - T - borrow);   digit = signed bit field 23..1 of (0 - nhi);  A' = A + (b << 4)

for torus words a, v that are multiples of 2^8 (every look-up table word the shifted kernel accepts is, and every
increment b << 12 keeps it so).  The 23-bit digit must be the same and (A' + 1) << 8 must equal am' + 1."""
import numpy as np

U64 = np.uint64
M64 = (1 << 64) - 1


def _u64(xs):
    return np.array([int(x) & M64 for x in xs], dtype=U64)


def _general(am, vm, keep, b):
    t = np.where(keep, vm, ~vm)
    d = am - t - keep.astype(U64)
    nhi = (d >> U64(32)).astype(np.uint32)
    dig = (np.uint32(0xFF) - nhi).astype(np.int32) >> 9
    return dig, am + (b << U64(12))


def _shifted(A, V, keep, b):
    T = np.where(keep, V, ~V)
    d = A - T - keep.astype(U64)
    nhi = (d >> U64(32)).astype(np.uint32)
    y = np.uint32(0) - nhi
    field = ((y >> np.uint32(1)) & np.uint32(0x7FFFFF)).astype(np.int64)      # v_bfe_i32 y, 1, 23
    dig = np.where(field >= 1 << 22, field - (1 << 23), field).astype(np.int32)
    return dig, A + (b << U64(4))


def _check(a, v, keep, b, rng):
    """a, v: torus words (multiples of 2^8); keep: lanes NOT flipped; b: bits of a double in [1, 2]"""
    assert not ((a | v) & U64(0xFF)).any()
    am, vm = a - U64(1), v - U64(1)
    top = lambda n: rng.integers(0, 256, n).astype(U64) << U64(56)          # the top byte carries no meaning
    A = (am >> U64(8)) ^ top(len(a))
    V = (vm >> U64(8)) ^ top(len(a))
    with np.errstate(over="ignore"):
        dig, am2 = _general(am, vm, keep, b)
        dig_s, A2 = _shifted(A, V, keep, b)
        assert np.array_equal(dig_s, dig), np.nonzero(dig_s != dig)[0][:10]
        assert np.array_equal((A2 + U64(1)) << U64(8), am2 + U64(1))
        # ... and the digit is what it is meant to be: round(x / 2^41) of the difference x = +-v - a, wrapped to 23 bits
        x = np.where(keep, v, U64(0) - v) - a
        want = (((x >> U64(32)).astype(np.uint32) + np.uint32(0x100)).astype(np.int32) >> 9)
        assert np.array_equal(dig, want)
    return dig


def _doubles(rng, n):
    """bit patterns of 1 + f, f in [0, 1): exponent 0x3FF and any mantissa; 2.0 stands for a sum that rounded up"""
    return U64(0x3FF) << U64(52) | rng.integers(0, 1 << 52, n, dtype=np.int64).astype(U64)


def test_random_words_both_signs():
    rng = np.random.default_rng(0xACC)
    n = 200_000
    a = rng.integers(0, 1 << 56, n, dtype=np.int64).astype(U64) << U64(8)
    v = rng.integers(0, 1 << 56, n, dtype=np.int64).astype(U64) << U64(8)
    keep = rng.integers(0, 2, n).astype(bool)
    dig = _check(a, v, keep, _doubles(rng, n), rng)
    assert dig.min() < -(1 << 21) and dig.max() > (1 << 21) and keep.any() and not keep.all()


def test_difference_high_words_at_the_rounding_edges():
    """hi32 of the difference 0x7FFFFFxx (the rounding add wraps the digit from 2^22 - 1 to -2^22) and 0xFFFFFFxx (it
    carries -1 into 0), next to 0x7FFFFExx, 0x800000xx, 0x000000xx, 0x0000FFxx, 0x0001FFxx; kept and flipped lanes"""
    rng = np.random.default_rng(0xED6E)
    his = [h << 8 | xx for h in (0x7FFFFF, 0xFFFFFF, 0x7FFFFE, 0x800000, 0x000000, 0x0000FF, 0x0001FF, 0xFFFFFE)
           for xx in (0x00, 0x01, 0x7F, 0x80, 0xFF)]
    lows = [0x00000000, 0x00000100, 0x80000000, 0xFFFFFF00]
    a_s, v_s, k_s = [], [], []
    for hi in his:
        for lo in lows:
            x = hi << 32 | lo
            for a in [0, 1 << 8, M64 & ~0xFF, 1 << 63] + [int(r) << 8 for r in rng.integers(0, 1 << 56, 4, dtype=np.int64)]:
                for keep in (True, False):
                    v = (x + a) & M64 if keep else (-(x + a)) & M64      # x = +-v - a
                    a_s.append(a); v_s.append(v); k_s.append(keep)
    a, v, keep = _u64(a_s), _u64(v_s), np.array(k_s)
    dig = _check(a, v, keep, _doubles(rng, len(a)), rng)
    by_hi = {hi: set() for hi in his}
    for k, d in enumerate(dig):
        by_hi[his[k // (len(lows) * 8 * 2)]].add(int(d))
    assert by_hi[0x7FFFFF00] == {-(1 << 22)} and by_hi[0x7FFFFE00] == {(1 << 22) - 1}
    assert by_hi[0xFFFFFFFF] == {0} and by_hi[0xFFFFFE80] == {-1} and by_hi[0x0000FF00] == {128}


def test_update_with_extreme_mantissas():
    """b = 1.0, all-ones mantissa, 2.0 (1 + f rounded up: the increment is 0 mod 2^64 in both forms), one unit;
    accumulators about to carry out of the 56 kept bits, and out of the low word"""
    rng = np.random.default_rng(0xB17)
    bs = [0x3FF0000000000000, 0x3FFFFFFFFFFFFFFF, 0x4000000000000000, 0x3FF0000000000001, 0x3FF8000000000000,
          0x3FF00000FFFFFFFF, 0x3FF0000100000000]
    accs = [0, 1 << 8, M64 & ~0xFF, M64 & ~0xFFF, 0xFFFFFFFF00, 0xFFFFF000, 1 << 63, (1 << 63) - (1 << 12)]
    a = _u64([x for x in accs for _ in bs])
    b = _u64([y for _ in accs for y in bs])
    v = rng.integers(0, 1 << 56, len(a), dtype=np.int64).astype(U64) << U64(8)
    for keep in (np.ones(len(a), bool), np.zeros(len(a), bool)):
        _check(a, v, keep, b, rng)


def test_a_long_run_keeps_the_two_forms_in_step():
    """742 updates in a row from look-up-table-like words (multiples of 2^59), digits taken against a rotated copy of
    the running accumulator like the kernel's rotated read; the top byte is scrambled again after every step"""
    rng = np.random.default_rng(0x10AD)
    n = 2048
    x = rng.integers(0, 32, n).astype(U64) << U64(59)
    am = x - U64(1)
    A = am >> U64(8)
    with np.errstate(over="ignore"):
        for i in range(742):
            s = int(rng.integers(1, 4096))
            keep = (np.arange(n) >= (s & 2047)) != (s >= 2048)
            vm, V = np.roll(am, s & 2047), np.roll(A, s & 2047)
            b = _doubles(rng, n)
            A ^= rng.integers(0, 256, n).astype(U64) << U64(56)
            dig, am = _general(am, vm, keep, b)
            dig_s, A = _shifted(A, V, keep, b)
            assert np.array_equal(dig, dig_s), i
        assert np.array_equal((A + U64(1)) << U64(8), am + U64(1))
        assert not ((am + U64(1)) & U64(0xFFF)).any()
