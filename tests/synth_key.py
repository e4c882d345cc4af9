"""Synthetic, noise-free bootstrapping keys whose polynomials are monomials, and integer references of a whole blind
rotation under them (test infrastructure; numpy only, nothing from oracle/ or the library).

GGSW i is bits[i] * G + Z_i with G = diag(2^41) (one level, base 2^23) and Z_i two noise-free GLWE encryptions of zero
(A, A * S) under S = X^js, A = c * X^k, c = (odd integer < 1024) * 2^41.  An external product with such a key is a few
negacyclic rotations and scalings in wrapping uint64, so the references below use no transform at all.  Every key word
is a multiple of 2^41: the 2^6 / 2^7 grid roundings at key load are the identity (offgrid_material() below adds an
offset to every word, so that they are not), every product is far inside the exact
kernels' CRT range, and the low 41 bits of every accumulator coefficient never change -- a look-up table whose low 41
bits sit on the decomposition's edges keeps its exact ties through every iteration of a row.

Bounds of the f64 arithmetics against the integer references on rows with ONE product (the digits are integers before
the transform, so the only difference is the f64 rounding of that product), measured on the CPU mirrors (oracle modes 3
and 4, bit-identical to the kernels) over the committed row set:
    mode 3 (f64 FFT)          max |mirror - reference| = 2^23.70
    mode 4 (f64 FFT, two-bit) max |mirror - reference| = 2^24.58
T3 and T4 are 8 x those; a single wrong digit moves a coefficient by at least 2^41, more than 2^10 above either.
The same on the rows whose last step is their one product with a GGSW of uniformly random 64-bit words (class U of
offgrid_material(); measured by tests/test_key_load.py against the integer reference):
    mode 3 (f64 FFT)          max |mirror - reference| = 2^40.56
    mode 4 (f64 FFT, two-bit) max |mirror - reference| = 2^41.78
T3U and T4U are 8 x those.  A key word of 2^63 times a digit of 2^22 has an f64 ulp of 2^33: the bound is one on the
rounding of a last product, as T3X / T4X, not on a digit."""
import functools

import numpy as np

N = 2048
LWE_N = 742
U = np.uint64
G41 = 1 << 41

T3 = 8 * 2 ** 23.70
T4 = 8 * 2 ** 24.58
MIN_TIES_PER_PRODUCT = 128

EXPONENTS = (1, 2, 31, 32, 63, 64, 65, 127, 1023, 1024, 2047, 2048, 2049, 2111, 4032, 4095)
EDGE_LOW = (0, 1, (1 << 40) - 1, 1 << 40, (1 << 40) + 1, (1 << 41) - 1)
PAIR_SHAPES = ((65, 0), (0, 2111), (31, 31), (2049, 4095), (3000, 1096), (2048, 2048), (1, 4095), (1023, 1024))
ROWS_SEED = 0x5E7B17
_ARANGE = np.arange(N, dtype=np.int64)


def rot(p, a):
    """X^a * p mod (X^2048 + 1), a in [0, 4096): an index gather, negated where the index wrapped."""
    j = (_ARANGE - int(a)) & (2 * N - 1)
    v = p[j & (N - 1)]
    return np.where(j >= N, U(0) - v, v)


def digit(x, rounding=1 << 40):
    """Closest multiple of 2^41 as a signed 23-bit digit, in two's complement uint64 (ties round up)."""
    v = ((x + U(rounding)) >> U(41)) & U((1 << 23) - 1)
    return v - ((v >> U(22)) << U(23))


def digit_ties_down(x):
    """The mutant of the reference's own mutation check: exact ties round the other way."""
    return digit(x, (1 << 40) - 1)


def mod_switch(x):
    """The kernels' modulus switch of a torus word to [0, 4096)."""
    return (((np.asarray(x, U) + U(1 << 51)) >> U(52)) & U(4095)).astype(np.uint32)


def sample_extract(acc):
    """[2, 2048] accumulator -> LWE [2049] of coefficient 0."""
    out = np.zeros(N + 1, U)
    out[0] = acc[0][0]
    out[1:N] = U(0) - acc[0][N - 1:0:-1]
    out[N] = acc[1][0]
    return out


def monomial_key(n_ggsw, bits, rng, js=5):
    """-> key [n_ggsw][row 2][col 2][2048] u64 and its description {(i, row, col): [(coef, exponent), ...]}."""
    key = np.zeros((n_ggsw, 2, 2, N), U)
    desc = {}
    for i in range(n_ggsw):
        for row in range(2):
            c = (2 * int(rng.integers(0, 512)) + 1) << 41
            k = int(rng.integers(0, 2 * N))
            for col in range(2):
                mono = [(c, (k + js * col) & (2 * N - 1))]
                if bits[i] and row == col:
                    mono.append((G41, 0))
                desc[(i, row, col)] = mono
                for coef, e in mono:          # exponents >= 2048 store the negated coefficient at e - 2048
                    w = int(key[i, row, col, e & (N - 1)]) + (coef if e < N else -coef)
                    key[i, row, col, e & (N - 1)] = U(w & ((1 << 64) - 1))
    return key, desc


def pair_bits(s):
    """Messages of the pair key: s(1-s'), (1-s)s', s s' per pair (s, s') = (s[2p], s[2p+1]), flat [371 * 3]."""
    a, b = np.asarray(s[0::2], np.int64), np.asarray(s[1::2], np.int64)
    return np.stack([a * (1 - b), (1 - a) * b, a * b], axis=1).reshape(-1)


def negacyclic_matrix(d):
    """[2048][2048], T[n][j] = d[n - j], negated where the index wrapped: T @ k is the negacyclic product d * k.  A
    strided view of (-d[1:], d), nothing is copied."""
    ext = np.concatenate([-d[1:], d])
    return np.lib.stride_tricks.as_strided(ext[N - 1:], (N, N), (ext.strides[0], -ext.strides[0]), writeable=False)


def dense_product(key_g, d):
    """Schoolbook external product of the digits d [2][2048] with a dense GGSW [row 2][col 2][2048] in wrapping uint64."""
    out = np.zeros((2, N), U)
    for row in range(2):
        if d[row].any():
            out += (negacyclic_matrix(d[row]) @ key_g[row].T).T
    return [out[0], out[1]]


def _product(desc, g, d, dense=None, log=None, used=None):
    """Sparse external product of the digits d [2][2048] with GGSW g -> [2][2048]; GGSWs in `dense` {g: [2][2][2048]}
    are multiplied out in full, and (g, d) is appended to `log`.  used: a set that receives (g, row) for every GGSW
    row that meets a non-zero digit."""
    if used is not None:
        used.update((g, row) for row in range(2) if d[row].any())
    if dense is not None and g in dense:
        if log is not None:
            log.append((g, np.stack(d)))
        return dense_product(dense[g], d)
    out = [np.zeros(N, U), np.zeros(N, U)]
    for col in range(2):
        for row in range(2):
            for coef, e in desc[(g, row, col)]:
                out[col] = out[col] + U(coef) * rot(d[row], e)
    return out


def _start(ms, lut):
    return [np.zeros(N, U), rot(np.asarray(lut, U), (2 * N - int(ms[LWE_N])) & (2 * N - 1))]


def blind_rotate_ref(desc, ms, lut, digit=digit, ties=None, dense=None, log=None, used=None):
    """Classic blind rotation, ACC += GGSW_i (.) (X^a ACC - ACC) per mask element a = ms[i] != 0 -> [2, 2048].
    ties: a list that receives, per product, the number of body differences whose low 41 bits equal 2^40."""
    acc = _start(ms, lut)
    for i in range(LWE_N):
        a = int(ms[i])
        if a == 0:
            continue
        diff = [rot(acc[r], a) - acc[r] for r in range(2)]
        if ties is not None:
            ties.append(int(np.count_nonzero((diff[1] & U((1 << 41) - 1)) == U(1 << 40))))
        p = _product(desc, i, [digit(x) for x in diff], dense, log, used)
        acc = [acc[c] + p[c] for c in range(2)]
    return np.stack(acc)


def blind_rotate_mb2_ref(desc, ms, lut, digit=digit, dense=None, log=None, used=None):
    """Two key bits per step: ACC += sum_t (X^e_t - 1) (K_t (.) ACC), t over (e1, e2, e1 + e2) -> [2, 2048]."""
    acc = _start(ms, lut)
    for p in range(LWE_N // 2):
        e1, e2 = int(ms[2 * p]), int(ms[2 * p + 1])
        if (e1 | e2) == 0:
            continue
        d = [digit(x) for x in acc]
        new = list(acc)
        for t, e in enumerate((e1, e2, (e1 + e2) & (2 * N - 1))):
            pt = _product(desc, 3 * p + t, d, dense, log, used)
            new = [new[c] + rot(pt[c], e) - pt[c] for c in range(2)]
        acc = new
    return np.stack(acc)


def centred_abs_max(a, b):
    """max |a - b| over all words, the difference taken mod 2^64 and centred."""
    return int(np.abs((np.asarray(a, U) - np.asarray(b, U)).view(np.int64).astype(np.float64)).max())


def msg_lut():
    """The `msg` look-up table (v & 3 at Delta = 2^59, 16 boxes of 128, rotated by half a box)."""
    tmp = np.repeat((np.arange(16, dtype=U) & U(3)) << U(59), N // 16)
    return np.concatenate([tmp[64:], U(0) - tmp[:64]])


def _torus(a, variant):
    """A torus word that the modulus switch takes to a: exact, just below the upper edge, or exactly on the lower edge
    (a = 0 on the lower edge is 0xFFF8000000000000, which rounds to 4096 and must act as 0; a = 4095 below the upper
    edge is 0xFFF7FFFFFFFFFFFF)."""
    a = int(a)
    if variant == 1:
        return (a << 52) + (1 << 51) - 1
    if variant == 2:
        return (((a - 1) & 4095) << 52) + (1 << 51)
    return a << 52


class Material:
    """Key bits, both keys with their descriptions, and the fixed row set."""


@functools.lru_cache(maxsize=None)
def material():
    rng = np.random.default_rng(ROWS_SEED)
    m = Material()
    m.js = 5
    m.s = rng.integers(0, 2, LWE_N).astype(np.int64)
    m.bsk, m.desc = monomial_key(LWE_N, m.s, rng, m.js)
    m.bsk_mb2, m.desc_mb2 = monomial_key(3 * (LWE_N // 2), pair_bits(m.s), rng, m.js)

    edge = [rng.choice(np.array(EDGE_LOW, U), N) + (rng.integers(0, 1 << 23, N).astype(U) << U(41)) for _ in range(2)]
    m.luts = np.stack(edge + [np.full(N, 1 << 62, U), msg_lut()])
    E0, E1, CONST, MSG = 0, 1, 2, 3
    by_bit = [np.flatnonzero(m.s == 0), np.flatnonzero(m.s == 1)]
    rows, lut_idx, kinds = [], [], []

    def add(kind, row, lut):
        rows.append(np.array(row, dtype=U)); lut_idx.append(lut); kinds.append(kind)

    def blank(n_as_zero=0):
        """All-zero mask; n_as_zero elements hold words that are not 0 but switch to 0."""
        row = [0] * (LWE_N + 1)
        for i in rng.choice(LWE_N, n_as_zero, replace=False):
            row[int(i)] = (0xFFF8000000000000, (1 << 51) - 1)[int(i) & 1]
        return row

    # one product each: every exponent once in a mask element (key bit 0 for even k, 1 for odd k) and once in a body
    for k, e in enumerate(EXPONENTS):
        row = blank(6 if k % 4 == 3 else 0)
        row[int(rng.choice(by_bit[k & 1]))] = _torus(e, k % 3)
        row[LWE_N] = _torus(EXPONENTS[(7 * k + 3) % 16], (k + 1) % 3)
        add("single", row, (E0, E1)[(k >> 1) & 1])
    for bit in range(2):                       # the constant LUT under X^2048: the digit -2^22 in every coefficient
        row = blank()
        row[int(rng.choice(by_bit[bit]))] = _torus(2048, 2 * bit)
        row[LWE_N] = _torus((0, 77)[bit], 2 - 2 * bit)
        add("single", row, CONST)
    # one pair each (two classic products, one two-bit product): the pair shapes of the two-bit kernels
    for k, (e1, e2) in enumerate(PAIR_SHAPES):
        row = blank()
        p = int(rng.integers(0, LWE_N // 2))
        row[2 * p], row[2 * p + 1] = _torus(e1, k % 3) if e1 else 0, _torus(e2, (k + 1) % 3) if e2 else 0
        row[LWE_N] = _torus(int(rng.integers(0, 4096)), k % 3)
        add("pair", row, (E0, E1)[k & 1])
    # 24 non-zero elements: 8 of the exponents at elements of a chosen key bit, their pair partners, 8 anywhere
    for r in range(40):
        row = blank(4 if r % 5 == 0 else 0)
        used = set()
        for t in range(8):
            while True:
                i = int(rng.choice(by_bit[((r >> 1) + t) & 1]))
                if i not in used and (i ^ 1) not in used:
                    break
            used.update((i, i ^ 1))
            row[i] = _torus(EXPONENTS[(8 * r + t) % 16], (r + t) % 3)
            row[i ^ 1] = _torus(int(rng.integers(1, 4096)), 0)
        while len(used) < 24:
            i = int(rng.integers(0, LWE_N))
            if i not in used:
                used.add(i)
                row[i] = int(rng.integers(1 << 51, (1 << 64) - (1 << 51), dtype=U))         # switches to 1..4095
        body = EXPONENTS[r] if r < 16 else int(rng.integers(0, 4096))
        row[LWE_N] = (0xFFF8000000000000, 0xFFF7FFFFFFFFFFFF)[r & 1] if r in (16, 17) else _torus(body, r % 3)
        add("sparse", row, (E0, E1, E0, E1, E0, E1, MSG, CONST)[r % 8])
    # 742 random elements: full 64-bit torus words
    for r in range(4):
        add("full", rng.integers(0, 1 << 64, LWE_N + 1, dtype=U), (E0, E1, MSG, E1)[r])
    add("zero", blank(), E0)
    row = blank(8); row[LWE_N] = _torus(1023, 1)
    add("zero", row, E1)

    m.ks = np.stack(rows)
    m.ms = mod_switch(m.ks)
    m.lut_idx = np.array(lut_idx, np.uint32)
    m.kinds = kinds
    for a in (m.s, m.bsk, m.bsk_mb2, m.luts, m.ks, m.ms, m.lut_idx):
        a.setflags(write=False)
    return m


def rows_of(m, *kinds):
    return [r for r, k in enumerate(m.kinds) if k in kinds]


class References:
    """acc, acc_mb2 [R][2][2048]: accumulators of the classic and the two-bit integer reference on the row set; out,
    out_mb2 [R][2049]: their sample extractions; ties: exact ties per product over all products of the classic rows."""


@functools.lru_cache(maxsize=None)
def references():
    m = material()
    ref = References()
    ref.ties = []
    ref.acc = np.stack([blind_rotate_ref(m.desc, m.ms[r], m.luts[m.lut_idx[r]], ties=ref.ties) for r in range(len(m.ks))])
    ref.acc_mb2 = np.stack([blind_rotate_mb2_ref(m.desc_mb2, m.ms[r], m.luts[m.lut_idx[r]]) for r in range(len(m.ks))])
    ref.out = np.stack([sample_extract(a) for a in ref.acc])
    ref.out_mb2 = np.stack([sample_extract(a) for a in ref.acc_mb2])
    for a in (ref.acc, ref.acc_mb2, ref.out, ref.out_mb2):
        a.setflags(write=False)
    return ref


def dense_case():
    """The chosen masks for a real dense key: the rows of at most 24 products (schoolbook stays affordable), every one
    with an edge LUT, so that the first product of every row decomposes exact ties under full-magnitude key
    coefficients -> (ks [n][743], ms [n][743], lut_idx [n]); the LUTs are material().luts."""
    m = material()
    rows = rows_of(m, "single", "pair", "sparse")
    return m.ks[rows], m.ms[rows], (m.lut_idx[rows] & np.uint32(1))


# ---- keyswitch under a synthetic key ---------------------------------------------------------------------------------
#
# ks[j] = b * [j == 742] - sum_{i < 2048, l < 5} d(i, l) * KSK[5 i + l][j] in wrapping uint64, of which the library only
# ever shows (ks + 2^51) >> 52.  The key below makes all 64 bits decide those 12:
#   * top part: column j < 742 owns one input coefficient top[j] with KSK[(top[j], l)][j] = -2^(61 - 3 l) and zero in
#     every other column, so the column's output carries that coefficient's 15-bit rounding v in bits 49..63; v = 4 mod 8
#     is an odd multiple of 2^51, a modulus-switch edge (column 742: the body is one);
#   * dense part: the other 1306 coefficients hold full 64-bit words in every column -- one of 32 word rows (balanced bytes
#     -128 and 127 in every plane, carries that run through all planes, random words), the same in all five levels except
#     that one level, the twin, holds the word + 1.  Digits that sum to zero over a coefficient's five levels cancel
#     exactly mod 2^64 and leave minus the twin's digit in every column at once.
# An "edge" row therefore has all 743 outputs at edge + r, r in {0, -1, +1} its residual: one unit of error of either
# sign in any byte plane of any key word with a non-zero digit changes a visible value on a row with r = 0 or r = -1.
KS_N, KS_LEVELS, KS_COLS = 2048, 5, 743
KS_SEED = 0x4B5EED
KS_ROWS = 63                      # odd: a row changes its position in a tile of 32 between the repeats of a batch
KS_WIDTHS = (1, 128, 129, 300, 600, 1281, 2817)
KS_GROUPS = 32
KS_SPECIAL = tuple(0x80 << 8 * b for b in range(8)) + tuple(0x7F << 8 * b for b in range(8)) + (
    0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0xFFFFFFFFFFFFFFFF, 0x0000000000000080)
_M64 = (1 << 64) - 1


def ks_digits(a, rounding=1 << 48):
    """[..., 2048] torus words -> [..., 10240] int64 digits at index 5 i + l: 15-bit rounding (the sum wraps: words
    >= 2^64 - 2^48 round to zero), five balanced base-8 digits, least significant level (l = 4) first with carry, top
    carry dropped."""
    v = ((np.asarray(a, U) + U(rounding)) >> U(49)).astype(np.int64)
    out = np.empty(v.shape + (KS_LEVELS,), np.int64)
    for l in range(KS_LEVELS - 1, -1, -1):
        d = v & 7
        v >>= 3
        high = d >= 4
        out[..., l] = d - 8 * high
        v += high
    return out.reshape(v.shape[:-1] + (-1,))


def keyswitch_ref(ksk, cts, rounding=1 << 48, cols=slice(None)):
    """cts [R][2049], ksk [10240][743] -> ks [R][743] (or the chosen columns) in wrapping uint64."""
    d = ks_digits(cts[:, :KS_N], rounding).view(U)
    out = U(0) - d @ ksk[:, cols]
    body = np.zeros(KS_COLS, U)
    body[KS_COLS - 1] = 1
    return out + cts[:, KS_N:] * body[cols]


def balanced_bytes(w):
    """[...] uint64 -> [..., 8] int8 with w = sum_b s_b 2^(8 b) mod 2^64, s_b in [-128, 127]."""
    w = np.array(w, U)
    out = np.empty(w.shape + (8,), np.int8)
    for b in range(8):
        s = (w & U(0xFF)).astype(np.uint8).view(np.int8)
        out[..., b] = s
        w = (w - s.astype(np.int64).view(U)) >> U(8)
    return out


def ks_word(digits, low=0):
    """The torus word whose digits are `digits` [5] (most significant level first) and whose distance to the 15-bit grid
    is low in [-2^48, 2^48)."""
    v = sum(int(d) << 3 * (KS_LEVELS - 1 - l) for l, d in enumerate(digits)) & 0x7FFF
    return ((v << 49) + int(low)) & _M64


def ks_launch_shape(B, cus=256):
    """What launch_keyswitch_mfma (ks_kernels.hip) does with B rows on `cus` CUs: ("split-k", workgroups per split,
    splits) below 129 rows, else ("ring", unsliced tiles, sliced tiles, slices of K per sliced tile)."""
    if B < 129:
        tgroups, splits = ((B + 31) // 32 + 3) // 4, 1
        while splits < 16 and tgroups * 24 * splits < 256:
            splits *= 2
        return ("split-k", tgroups * 24, splits)
    tiles = 24 * ((B + 255) // 256)
    full = tiles // cus * cus
    rem, slices = tiles - full, 1
    if rem:
        slices = next((c for c in (8, 4, 2) if rem * c <= cus), 1)
    if slices == 1:
        full, rem = tiles, 0
    return ("ring", full, rem, slices)


# the launch shapes of KS_WIDTHS on 256 CUs; tests/test_gpu_synth_key.py leaves out a width whose shape differs elsewhere
KS_SHAPES_256 = {1: ("split-k", 24, 16), 128: ("split-k", 24, 16), 129: ("ring", 0, 24, 8), 300: ("ring", 0, 48, 4),
                 600: ("ring", 0, 72, 2), 1281: ("ring", 144, 0, 1), 2817: ("ring", 256, 32, 8)}


def ks_batch(n):
    """The row that each of the n ciphertexts of a batch repeats."""
    return np.arange(n) % KS_ROWS


class KsMaterial:
    """ksk [10240][743]; top [742]: the input coefficient of each column; dense [1306], group, twin: the other
    coefficients, their word row and twin level; cts [63][2049], kinds, residual (edge and input rows)."""


def _zero_sum_digits(rng, twin, rho):
    """[n][5] digits in [-4, 3] that sum to zero per coefficient, with -rho at the twin level."""
    n = len(twin)
    d = np.zeros((n, KS_LEVELS), np.int64)
    todo = np.arange(n)
    while len(todo):
        free = rng.integers(-4, 4, (len(todo), KS_LEVELS))
        free[np.arange(len(todo)), twin[todo]] = -rho[todo]
        last = (twin[todo] + 1) % KS_LEVELS                      # the level that closes the sum
        free[np.arange(len(todo)), last] = 0
        free[np.arange(len(todo)), last] = -free.sum(axis=1)
        ok = (free[np.arange(len(todo)), last] >= -4) & (free[np.arange(len(todo)), last] <= 3)
        d[todo[ok]] = free[ok]
        todo = todo[~ok]
    return d


@functools.lru_cache(maxsize=None)
def keyswitch_material():
    rng = np.random.default_rng(KS_SEED)
    m = KsMaterial()
    perm = rng.permutation(KS_N)
    m.top, m.dense = perm[:KS_COLS - 1], np.sort(perm[KS_COLS - 1:])
    n_dense = len(m.dense)
    ksk = np.zeros((KS_N, KS_LEVELS, KS_COLS), U)
    for l in range(KS_LEVELS):
        ksk[m.top, l, np.arange(KS_COLS - 1)] = U(-(1 << (61 - 3 * l)) & _M64)
    words = np.empty((KS_GROUPS, KS_COLS), U)
    special = np.array(KS_SPECIAL, U)
    for g in range(len(special)):                                # every column meets every special word
        words[g] = special[(g + np.arange(KS_COLS)) % len(special)]
    pool = np.array([0x80, 0x7F, 0xFF, 0x00], U)
    for g in range(len(special), KS_GROUPS):                     # random words, half of their bytes from the pool
        b = np.where(rng.integers(0, 2, (KS_COLS, 8)) == 1, pool[rng.integers(0, 4, (KS_COLS, 8))],
                     rng.integers(0, 256, (KS_COLS, 8)).astype(U))
        words[g] = (b << (U(8) * np.arange(8, dtype=U))).sum(axis=1, dtype=U)
    m.group = rng.integers(0, KS_GROUPS, n_dense)
    m.group[:KS_GROUPS] = np.arange(KS_GROUPS)
    m.twin = rng.integers(0, KS_LEVELS, n_dense)
    ksk[m.dense] = words[m.group][:, None, :]
    ksk[m.dense, m.twin] += U(1)
    m.ksk = ksk.reshape(KS_N * KS_LEVELS, KS_COLS)

    def dense_part(row, residual):
        """Digits that sum to zero over the five levels of every dense coefficient, so that the words cancel; the twins'
        digits are random too and sum to minus the residual over the row.  24 coefficients hold words that round to zero
        digits instead (wrapping ones among them)."""
        rho = rng.integers(-3, 4, n_dense)                       # minus the twin's digit
        quiet = rng.choice(n_dense, 24, replace=False)
        rho[quiet] = 0
        busy = np.setdiff1d(np.arange(n_dense), quiet)
        while rho.sum() != residual:
            i, step = int(rng.choice(busy)), (1 if rho.sum() < residual else -1)
            if -3 <= rho[i] + step <= 3:
                rho[i] += step
        d = _zero_sum_digits(rng, m.twin, rho)
        for k, i in enumerate(m.dense):
            row[i] = ks_word(d[k], int(rng.integers(-(1 << 48), 1 << 48)))
        wraps = (_M64 - (1 << 48) + 1, _M64, 0, (1 << 48) - 1)   # the first and last word that wrap, and that do not
        for k, i in enumerate(quiet):
            row[m.dense[i]] = wraps[k] if k < 4 else (int(rng.integers(-(1 << 48), 1 << 48)) & _M64)

    def top_part(row, r, input_edges):
        """v = 4 mod 8 on every column: an edge.  Distances to the grid: exact ties (low 49 bits 2^48, rounding up), the
        last word below a tie, on the grid, random.  input_edges: a quarter of the columns instead hold v = 3 mod 8 with
        the low 49 bits at 2^48 - 1 (one unit below the tie that would reach the edge) or a word that wraps to zero."""
        for j, i in enumerate(m.top):
            v = 8 * int(rng.integers(0, 4096)) + 4
            low = (-(1 << 48), (1 << 48) - 1, 0, int(rng.integers(-(1 << 48), 1 << 48)))[int(rng.integers(0, 4))]
            if input_edges and j % 4 == r % 4:
                if rng.integers(0, 4):
                    v, low = v - 1, (1 << 48) - 1
                else:
                    v, low = 0x7FFF, int(rng.integers(1 << 48, 1 << 49))   # >= 2^64 - 2^48
            row[i] = ((v << 49) + low) & _M64

    rows, kinds, residual = [], [], []
    for r in range(KS_ROWS):
        row = [0] * (KS_N + 1)
        row[KS_N] = (2 * int(rng.integers(0, 4096)) + 1) << 51   # the body: an edge
        if r == 0 or r == 32:                                    # every digit -4 / every digit 3
            kind, d = ("neg4", "pos3")[r // 32], (-4, 3)[r // 32]
            row[:KS_N] = [ks_word([d] * 5, int(rng.integers(-(1 << 48), 1 << 48))) for _ in range(KS_N)]
        elif r == 1:
            kind = "zero"                                        # a trivial ciphertext
        elif r in (16, 17, 48, 49):
            kind = "full"
            row[:] = [int(x) for x in rng.integers(0, 1 << 64, KS_N + 1, dtype=U)]
        else:
            kind = ("edge", "input")[r & 1]
            residual.append((r, (0, -1, 1)[(r // 2) % 3]))
            dense_part(row, residual[-1][1])
            top_part(row, r, kind == "input")
        rows.append(np.array(row, dtype=U))
        kinds.append(kind)
    m.cts, m.kinds, m.residual = np.stack(rows), kinds, dict(residual)
    for a in (m.ksk, m.cts, m.top, m.dense, m.group, m.twin):
        a.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def keyswitch_reference():
    """ks [63][743] in all 64 bits (3.5 s of uint64 matmul, once per process)."""
    m = keyswitch_material()
    ks = keyswitch_ref(m.ksk, m.cts)
    ks.setflags(write=False)
    return ks


# ---- the exact kernels near the top of their CRT range ---------------------------------------------------------------
#
# A few GGSWs of the classic key and the matching triples of the pair key are dense with every coefficient at full
# magnitude: the words 2^63 (centred: -2^63) and 2^63 - 2^7 (on the 2^6 grid of the classic key and the 2^7 grid of the
# pair key), with the signs aligned against the negacyclic wrap so that the terms of one chosen coefficient all add.
# Under a constant look-up table -- 2^62 for the classic arithmetic, whose digits are those of X^2048 ACC - ACC = -2^63,
# and 2^63 for the two-bit one, whose digits are those of ACC itself -- every body digit is -2^22.  In the two-step rows
# a first, monomial step (GGSW 100 / pair 50, whose mask polynomial holds c = odd * 2^40) leaves the mask at an odd
# multiple of 2^62 (classic) / at 2^63 (two-bit) everywhere, so that both rows of the dense GGSW get the digit -2^22.
# Largest product coefficient, as a true integer in units of the key grid (tests/test_synth_key.py prints them):
#     classic kernel, one-step rows   2^90.00   (2048 * 2^22 * 2^57)
#     classic kernel, two-step rows   2^91.00   the bound stated for blind_rotate_kernel, reached exactly
#     two-bit kernel, one-pair rows   2^91.00   (2048 * 2^22 * 4 * 2^56: e1 = e2 = 2048 cancels the third key)
#     two-bit kernel, two-step rows   2^92.00   against the stated 2^92.6 and a CRT range of p0 p1 / 2 = 2^93.0
# The f64 arithmetics on the same rows, CPU mirrors (bit-identical to the kernels) against the integer references, on the
# rows whose last step is their one dense product:
#     mode 3 (f64 FFT)          max |mirror - reference| = 2^45.58
#     mode 4 (f64 FFT, two-bit) max |mirror - reference| = 2^48.00
# T3X and T4X are 8 x those, for the reason given at T3 / T4.  Both are ABOVE one digit step of 2^41 (a product of 2^96
# to 2^99 in torus units has an f64 ulp of 2^44 to 2^47): where another step follows a dense product the digits of that
# step differ from the integer reference's and the distance is no longer a rounding error (2^52.42 measured); those rows
# are held to the mirrors bit for bit like all others, and to no distance.
X_DENSE = (400, 401, 600)          # classic GGSWs; the pair triples are those of the pairs 200 and 300
X_PAIRS = (200, 300)
X_FIRST, X_FIRST_PAIR = 100, 50    # the first step of the two-step rows
X_SEED = 0xE87E3E
NTT_P0, NTT_P1 = 0x7FFFFFFEC001, 0x7FFFFFFE7001
K_NEG, K_POS = 1 << 63, (1 << 63) - (1 << 7)
T3X = 8 * 2 ** 45.58
T4X = 8 * 2 ** 48.00


def _aligned(n_star, sign):
    """A full-magnitude polynomial whose terms in coefficient n_star of a product with constant digits all add:
    sign * magnitude up to n_star, the opposite sign beyond (those terms wrap and are negated)."""
    lo, hi = (K_NEG, K_POS) if sign < 0 else (K_POS, K_NEG)
    return np.where(_ARANGE <= n_star, U(lo), U(hi))


def dense_product_true(key_g, d, grid_bits):
    """The same product as true integers in units of 2^grid_bits, key words centred -> [2][2048] Python integers.
    Three 20-bit limbs of the key keep every partial sum below 2^54."""
    kc = key_g.view(np.int64) >> grid_bits
    limbs = [kc & ((1 << 20) - 1), (kc >> 20) & ((1 << 20) - 1), kc >> 40]
    parts = [np.zeros((2, N), np.int64) for _ in limbs]
    for row in range(2):
        if d[row].any():
            t = negacyclic_matrix(d[row].view(np.int64))
            for part, limb in zip(parts, limbs):
                part += (t @ limb[row].T).T
    return sum(part.astype(object) << (20 * k) for k, part in enumerate(parts))


def wrap_to_range(x, modulus, grid_bits):
    """What a CRT of range `modulus` would make of the true integers x: the representative in (-M/2, M/2], then the
    torus word x * 2^grid_bits mod 2^64."""
    out = np.empty(x.shape, U)
    for idx, v in np.ndenumerate(x):
        v = int(v) % modulus
        if v > modulus // 2:
            v -= modulus
        out[idx] = (v << grid_bits) & _M64
    return out


def _set_mono(key, desc, where, mono):
    key_poly = key[where[0], where[1], where[2]]
    key_poly[:] = 0
    desc[where] = mono
    for coef, e in mono:
        w = int(key_poly[e & (N - 1)]) + (coef if e < N else -coef)
        key_poly[e & (N - 1)] = U(w & _M64)


class ExtremeMaterial:
    """bsk, bsk_mb2 with their descriptions and dense {g: [2][2][2048]} / dense_mb2 {3 p + t: ...}; luts [2][2048]:
    constant 2^62, constant 2^63; ks [R][743], ms, lut_idx, kinds ("one", "pair", "two"), one_dense, one_dense_mb2."""


@functools.lru_cache(maxsize=None)
def extreme_material():
    base = material()
    rng = np.random.default_rng(X_SEED)
    x = ExtremeMaterial()
    x.bsk, x.bsk_mb2 = base.bsk.copy(), base.bsk_mb2.copy()
    x.desc, x.desc_mb2 = dict(base.desc), dict(base.desc_mb2)
    # dense GGSWs.  400 / pair 200, keys 1 and 2: every coefficient -2^63, all 2048 terms of coefficient 2047 add;
    # 401, 600 / the other triples: other aligned coefficients and signs per polynomial, and random signs
    n_stars = (N - 1, 0, 1023, 1024, 2046, 1, 777, N - 1)
    def ggsw(kind):
        g = np.empty((2, 2, N), U)
        for k in range(4):
            if kind == 0:
                g[k >> 1, k & 1] = K_NEG
            elif kind == 1:
                g[k >> 1, k & 1] = _aligned(n_stars[int(rng.integers(0, 8))], (-1, 1)[int(rng.integers(0, 2))])
            else:
                g[k >> 1, k & 1] = np.where(rng.integers(0, 2, N) == 1, U(K_NEG), U(K_POS))
        return g
    x.dense = {g: ggsw(k) for k, g in enumerate(X_DENSE)}
    x.dense_mb2 = {3 * p + t: ggsw((0, 0, 1, 1, 2, 1)[3 * k + t]) for k, p in enumerate(X_PAIRS) for t in range(3)}
    for g, poly in x.dense.items():
        x.bsk[g] = poly
    for g, poly in x.dense_mb2.items():
        x.bsk_mb2[g] = poly
    # first steps: c = odd * 2^40 in the polynomial that takes the body digits into the mask
    for key, desc, g in ((x.bsk, x.desc, X_FIRST), (x.bsk_mb2, x.desc_mb2, 3 * X_FIRST_PAIR)):
        _set_mono(key, desc, (g, 1, 0), [((2 * int(rng.integers(0, 512)) + 1) << 40, int(rng.integers(0, 2 * N)))])

    x.luts = np.stack([np.full(N, 1 << 62, U), np.full(N, 1 << 63, U)])
    masks = [("one", {400: 2048}), ("one", {401: 2048}), ("one", {600: 2048}), ("one", {400: 1}), ("one", {401: 1024}),
             ("one", {600: 4095}), ("one", {400: 2047}), ("one", {601: 2048}),
             ("pair", {400: 2048, 401: 2048}), ("pair", {400: 2048, 401: 1}), ("pair", {600: 2048, 601: 2048}),
             ("pair", {600: 2049, 601: 2047}), ("pair", {400: 2048, 401: 4095}),
             ("two", {100: 2048, 400: 2048}), ("two", {100: 2048, 400: 2048, 401: 2048}), ("two", {100: 2048, 600: 2048}),
             ("two", {100: 2048, 101: 2048, 600: 2048, 601: 2048})]
    rows, lut_idx, kinds = [], [], []
    for k, (kind, mask) in enumerate(masks):
        for lut in range(2):
            row = [0] * (LWE_N + 1)
            for i, e in mask.items():
                row[i] = _torus(e, (k + lut) % 3)
            row[LWE_N] = (0, 0xFFF8000000000000, (1 << 51) - 1)[k % 3]       # all three switch to 0
            rows.append(np.array(row, dtype=U)); lut_idx.append(lut); kinds.append(kind)
    x.ks = np.stack(rows)
    x.ms = mod_switch(x.ks)
    x.lut_idx = np.array(lut_idx, np.uint32)
    x.kinds = kinds
    # rows with ONE dense product, in the last step, in the classic / the two-bit arithmetic: where the f64 arithmetics
    # are bounded (the rounding of a dense product is above a digit step and changes the digits of any step after it)
    x.one_dense = [r for r in range(len(rows)) if np.count_nonzero(x.ms[r, list(X_DENSE)]) == 1
                   and int(np.flatnonzero(x.ms[r, :LWE_N])[-1]) in X_DENSE]
    x.one_dense_mb2 = [r for r in range(len(rows)) if sum(bool(x.ms[r, 2 * p] | x.ms[r, 2 * p + 1]) for p in X_PAIRS) == 1]
    for a in (x.bsk, x.bsk_mb2, x.luts, x.ks, x.ms, x.lut_idx):
        a.setflags(write=False)
    return x


class ExtremeReferences:
    """acc, acc_mb2 [R][2][2048], out, out_mb2 [R][2049] as in References; products, products_mb2: per row the dense
    products as (true integers in grid units [2][2048], the same product in wrapping uint64 [2][2048])."""


@functools.lru_cache(maxsize=None)
def extreme_references():
    x = extreme_material()
    ref = ExtremeReferences()
    ref.products, ref.products_mb2 = [], []
    acc, acc_mb2 = [], []
    for r in range(len(x.ks)):
        ms, lut = x.ms[r], x.luts[x.lut_idx[r]]
        log, log_mb2 = [], []
        acc.append(blind_rotate_ref(x.desc, ms, lut, dense=x.dense, log=log))
        acc_mb2.append(blind_rotate_mb2_ref(x.desc_mb2, ms, lut, dense=x.dense_mb2, log=log_mb2))
        ref.products.append([(dense_product_true(x.dense[g], d, 6), np.stack(dense_product(x.dense[g], d))) for g, d in log])
        found = []
        for (g, d), _, _ in zip(*[iter(log_mb2)] * 3):                # the three keys of a pair see the same digits
            p = g // 3
            e = (int(ms[2 * p]), int(ms[2 * p + 1]))
            # the combined key K1 (X^e1 - 1) + K2 (X^e2 - 1) + K3 (X^(e1+e2) - 1) of centred words in units of 2^7: below
            # 6 * 2^56
            comb = np.zeros((2, 2, N), np.int64)
            wrapping = np.zeros((2, N), U)
            for t, et in enumerate(e + ((e[0] + e[1]) & (2 * N - 1),)):
                k = x.dense_mb2[3 * p + t]
                kc = k.view(np.int64) >> 7
                j = (_ARANGE - et) & (2 * N - 1)
                comb += np.where(j >= N, -kc[..., j & (N - 1)], kc[..., j & (N - 1)]) - kc
                pt = dense_product(k, d)
                wrapping += np.stack([rot(pt[c], et) - pt[c] for c in range(2)])
            found.append((dense_product_true(comb.view(U), d, 0), wrapping))
        ref.products_mb2.append(found)
    ref.acc, ref.acc_mb2 = np.stack(acc), np.stack(acc_mb2)
    ref.out = np.stack([sample_extract(a) for a in ref.acc])
    ref.out_mb2 = np.stack([sample_extract(a) for a in ref.acc_mb2])
    for a in (ref.acc, ref.acc_mb2, ref.out, ref.out_mb2):
        a.setflags(write=False)
    return ref


def true_magnitude(products):
    """log2 of the largest |coefficient| over a row's dense products (grid units); -inf without one."""
    import math
    worst = max((abs(int(v)) for x_true, _ in products for v in x_true.ravel()), default=0)
    return math.log2(worst) if worst else float("-inf")


# ---- keys that do not lie on the key grid ----------------------------------------------------------------------------
#
# Key load rounds every word of the bootstrapping key to the nearest multiple of 2^6 (ties up, modulo 2^64), and every
# word of the pair key to 2^6 for the f64 arithmetic and -- from the ORIGINAL word -- to 2^7 for the exact one.  The keys
# below are material()'s plus an offset per word, in three classes of GGSW (a pair triple is three):
#   R "returns": every GGSW that is not M or U.  Offsets from R_OFFSETS; every word rounds back to material()'s word on
#     both grids, so the rows that meet only such GGSWs keep the outputs of references().  -1 and -32 on a zero word are
#     the words 2^64 - 1 and 2^64 - 32, which wrap to 0.
#   M "moves": the GGSWs of three one-product rows and of two two-product rows, and the pair triples at the same
#     positions (g // 2).  Offsets from M_OFFSETS: every word moves by +-2^6 or +-2^7 or stays, differently on the two
#     grids, and "6 then 7" differs from 7 on +32, +33, +63 (and on 2^63 - 33).  The rounded polynomial is dense, the
#     reference multiplies it out (dense= of _product).  Planted words: 2^64 - 32 and 2^64 - 1 (-> 0) in every
#     polynomial, 2^63 - 32 and 2^63 - 33 (-> 2^63, centred -2^63; the latter -> 2^63 - 2^6 on the 2^6 grid) in the
#     polynomials of GGSW row 0 only.  Row 0 meets the digits of the accumulator's mask, which are zero in the first
#     product of a row: the rows with one product never multiply a word of magnitude 2^63, whose f64 product has an ulp
#     of 2^33 and would leave T3 / T4 for the reason given at T3X; the second product of a two-product row and the
#     sparse and full rows do multiply them, where the exact kernels answer in every word and the f64 kernels to their
#     mirrors.
#   U "uniform": three GGSWs and two pair triples of uniformly random 64-bit words, as a foreign key has them.  No row of
#     material() but the full ones meets their mask elements, those are zeroed in the full rows here, and thirteen rows
#     of their own hold one or two products with them, four of them after a first step with a GGSW of class R, and
#     nothing else.  Where such a product is the row's only one with class U and its last step, the f64 arithmetics are
#     bounded against the integer reference by T3U / T4U (the module's docstring has the measured figures).
R_OFFSETS = (-32, -31, -1, 1, 31)
M_OFFSETS = (32, 33, 63, -33, -63, -64, 64, 95, 96)
M_PLANTS_WRAP = ((1 << 64) - 32, (1 << 64) - 1)
M_PLANTS_TOP = ((1 << 63) - 32, (1 << 63) - 33)
O_SEED = 0x0FF6E1D
T3U = 8 * 2 ** 40.56
T4U = 8 * 2 ** 41.78


def round_grid(x, bits):
    """The nearest multiple of 2^bits, ties up, modulo 2^64: what key load does to a key word."""
    return (np.asarray(x, U) + U(1 << (bits - 1))) & ~U((1 << bits) - 1)


def round_truncated(x, bits):
    return np.asarray(x, U) & ~U((1 << bits) - 1)


def round_ties_down(x, bits):
    return (np.asarray(x, U) + U((1 << (bits - 1)) - 1)) & ~U((1 << bits) - 1)


def round_6_then_7(x, bits):
    """The pair key's exact form taken from the words already rounded for the f64 form (on the 2^6 grid: no change)."""
    return round_grid(round_grid(x, 6), bits)


def round_wrong_grid(x, bits):
    """2^7 where 2^6 belongs, and the reverse."""
    return round_grid(x, 13 - bits)


# the mutants of the negative control (tests/test_key_load.py), as drop-in replacements of round_grid
ROUND_MUTANTS = {"truncation": round_truncated, "ties down": round_ties_down, "6 then 7": round_6_then_7,
                 "wrong grid": round_wrong_grid}


class OffgridMaterial:
    """bsk, bsk_mb2: the keys as they are loaded; desc, desc_mb2, luts: material()'s; m_dense, u_dense: the classic GGSWs
    of class M and U, m_pairs, u_pairs: the pairs whose triples are; blocked: the mask elements of the U GGSWs; ks, ms,
    lut_idx, kinds: material()'s rows (the full ones zero at `blocked`) and the "u" rows.  Row lists per arithmetic
    (classic / _mb2): r_rows meet GGSWs of class R only, m_rows one of class M at least; one_m: the rows with ONE product, which is
    with a GGSW of class M; one_u: the rows whose last step is their one product with a GGSW of class U."""


def _triples(pairs):
    return [3 * p + t for p in pairs for t in range(3)]


@functools.lru_cache(maxsize=None)
def offgrid_material():
    base = material()
    rng = np.random.default_rng(O_SEED)
    x = OffgridMaterial()
    x.desc, x.desc_mb2, x.luts = base.desc, base.desc_mb2, base.luts
    n_base = len(base.ks)
    first = lambda r: int(np.flatnonzero(base.ms[r, :LWE_N])[0])
    singles = [first(r) for r in rows_of(base, "single")][:3]
    doubles = [first(r) & ~1 for r in rows_of(base, "pair") if np.count_nonzero(base.ms[r, :LWE_N]) == 2][:2]
    x.m_dense = tuple(singles + [g + k for g in doubles for k in range(2)])
    x.m_pairs = tuple(sorted({g // 2 for g in x.m_dense}))
    light = rows_of(base, "single", "pair", "sparse", "zero")
    busy = (base.ms[light, :LWE_N] != 0).any(axis=0)
    free = [p for p in range(LWE_N // 2) if not (busy[2 * p] or busy[2 * p + 1]) and p not in x.m_pairs]
    x.u_pairs = tuple(free[:2])
    x.u_dense = (2 * free[0], 2 * free[0] + 1, 2 * free[1])
    x.blocked = tuple(2 * p + k for p in x.u_pairs for k in range(2))

    def shifted(key, m_idx, u_idx):
        raw = key + rng.choice(np.array(R_OFFSETS, np.int64), key.shape).view(U)
        for g in m_idx:
            raw[g] = key[g] + rng.choice(np.array(M_OFFSETS, np.int64), key[g].shape).view(U)
            for row in range(2):
                plants = (M_PLANTS_TOP + M_PLANTS_WRAP if row == 0 else M_PLANTS_WRAP + M_PLANTS_WRAP) * 2
                for col in range(2):
                    at = rng.choice(np.flatnonzero(key[g, row, col] == 0), len(plants), replace=False)
                    raw[g, row, col, at] = np.array(plants, U)
        for g in u_idx:
            raw[g] = rng.integers(0, 1 << 64, key[g].shape, dtype=U)
        return raw
    x.bsk = shifted(base.bsk, x.m_dense, x.u_dense)
    x.bsk_mb2 = shifted(base.bsk_mb2, _triples(x.m_pairs), _triples(x.u_pairs))

    ks = base.ks.copy()
    ks[:, list(x.blocked)] = 0                                   # changes the full rows only
    (a0, a1, b0, b1), E = x.blocked, EXPONENTS
    masks = [{g: E[(5 * k + 1) % 16]} for k, g in enumerate(x.u_dense * 2)] + [
        {b1: 2048}, {a0: 65, a1: 2111}, {b0: 4095, b1: 1}]
    # a first step with a GGSW of class R, so that GGSW row 0 of the U GGSW meets digits too.  These rows take the
    # constant and the `msg` look-up table: under an edge table the f64 rounding of the first step would decide exact
    # ties of the second, and the distance to the integer reference would be no rounding error (see T3X)
    x.u_first = next(g for g in range(LWE_N) if g // 2 not in x.m_pairs + x.u_pairs)
    two_step = [{x.u_first: E[(3 * k + 4) % 16], g: E[(7 * k + 2) % 16]} for k, g in enumerate(x.blocked)]
    rows, lut_idx = [], []
    for k, mask in enumerate(masks + two_step):
        row = [0] * (LWE_N + 1)
        for i, e in mask.items():
            row[i] = _torus(e, k % 3)
        row[LWE_N] = _torus(E[(3 * k + 2) % 16], (k + 1) % 3)
        rows.append(np.array(row, dtype=U)); lut_idx.append(k & 1 if k < len(masks) else 2 + (k & 1))
    x.ks = np.concatenate([ks, np.stack(rows)])
    x.ms = mod_switch(x.ks)
    x.lut_idx = np.concatenate([base.lut_idx, np.array(lut_idx, np.uint32)])
    x.kinds = list(base.kinds) + ["u"] * len(rows)

    on = x.ms[:, :LWE_N] != 0
    on_pair = on[:, 0::2] | on[:, 1::2]
    def split(on, m_idx, u_idx, one_kinds):
        hits_m = on[:, list(m_idx)].any(axis=1)
        r_rows = [r for r in range(n_base) if base.kinds[r] != "full" and not hits_m[r]]
        m_rows = [r for r in range(n_base) if hits_m[r]]
        one_m = [r for r in m_rows if base.kinds[r] in one_kinds]
        # the rows whose last step is their one product with a GGSW of class U
        one_u = [r for r in range(n_base, len(x.ks)) if on[r, list(u_idx)].sum() == 1 and int(np.flatnonzero(on[r])[-1]) in u_idx]
        return r_rows, m_rows, one_m, one_u
    x.r_rows, x.m_rows, x.one_m, x.one_u = split(on, x.m_dense, x.u_dense, ("single",))
    x.r_rows_mb2, x.m_rows_mb2, x.one_m_mb2, x.one_u_mb2 = split(on_pair, x.m_pairs, x.u_pairs, ("single", "pair"))
    for a in (x.bsk, x.bsk_mb2, x.ks, x.ms, x.lut_idx):
        a.setflags(write=False)
    return x


def offgrid_dense(x, pair_key, bits, rounding=round_grid, ggsws=None):
    """{g: the GGSW as key load leaves it on the 2^bits grid} for the GGSWs of class M and U of the classic key or the
    pair key, or for the given ones."""
    key = x.bsk_mb2 if pair_key else x.bsk
    if ggsws is None:
        ggsws = _triples(x.m_pairs + x.u_pairs) if pair_key else x.m_dense + x.u_dense
    return {g: rounding(key[g], bits) for g in ggsws}


def offgrid_row(x, r, pair_key, bits, rounding=round_grid, every=False, used=None):
    """The accumulator [2, 2048] of row r under the off-grid key rounded to 2^bits by `rounding`.  every: all GGSWs that
    the row meets are rounded from the loaded words and multiplied out (what a mutant needs, under which the words of
    class R do not return), not those of class M and U alone."""
    ggsws = None
    if every:
        on = np.flatnonzero(x.ms[r, :LWE_N])
        ggsws = _triples(sorted({int(i) // 2 for i in on})) if pair_key else [int(i) for i in on]
    dense = offgrid_dense(x, pair_key, bits, rounding, ggsws)
    if pair_key:
        return blind_rotate_mb2_ref(x.desc_mb2, x.ms[r], x.luts[x.lut_idx[r]], dense=dense, used=used)
    return blind_rotate_ref(x.desc, x.ms[r], x.luts[x.lut_idx[r]], dense=dense, used=used)


class OffgridReferences:
    """acc (the classic key on the 2^6 grid), acc_mb2_6, acc_mb2_7 (the pair key on either grid) [R][2][2048]; out,
    out_mb2_6, out_mb2_7 [R][2049]; used, used_mb2: the (GGSW, GGSW row) that met a non-zero digit on some row."""


@functools.lru_cache(maxsize=None)
def offgrid_references():
    x = offgrid_material()
    ref = OffgridReferences()
    ref.used, ref.used_mb2 = set(), set()
    dense, dense6, dense7 = offgrid_dense(x, False, 6), offgrid_dense(x, True, 6), offgrid_dense(x, True, 7)
    rows = range(len(x.ks))
    run = lambda r, dense, used: blind_rotate_mb2_ref(x.desc_mb2, x.ms[r], x.luts[x.lut_idx[r]], dense=dense, used=used)
    ref.acc = np.stack([blind_rotate_ref(x.desc, x.ms[r], x.luts[x.lut_idx[r]], dense=dense, used=ref.used) for r in rows])
    ref.acc_mb2_7 = np.stack([run(r, dense7, ref.used_mb2) for r in rows])
    ref.acc_mb2_6 = np.stack([ref.acc_mb2_7[r] if r in x.r_rows_mb2 else run(r, dense6, None) for r in rows])
    ref.out, ref.out_mb2_6, ref.out_mb2_7 = (np.stack([sample_extract(a) for a in acc])
                                             for acc in (ref.acc, ref.acc_mb2_6, ref.acc_mb2_7))
    for a in (ref.acc, ref.acc_mb2_6, ref.acc_mb2_7, ref.out, ref.out_mb2_6, ref.out_mb2_7):
        a.setflags(write=False)
    return ref
