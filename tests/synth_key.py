"""Synthetic, noise-free bootstrapping keys whose polynomials are monomials, and integer references of a whole blind
rotation under them (test infrastructure; numpy only, nothing from oracle/ or the library).

GGSW i is bits[i] * G + Z_i with G = diag(2^41) (one level, base 2^23) and Z_i two noise-free GLWE encryptions of zero
(A, A * S) under S = X^js, A = c * X^k, c = (odd integer < 1024) * 2^41.  An external product with such a key is a few
negacyclic rotations and scalings in wrapping uint64, so the references below use no transform at all.  Every key word
is a multiple of 2^41: the 2^6 / 2^7 grid roundings at key load are the identity, every product is far inside the exact
kernels' CRT range, and the low 41 bits of every accumulator coefficient never change -- a look-up table whose low 41
bits sit on the decomposition's edges keeps its exact ties through every iteration of a row.

Bounds of the f64 arithmetics against the integer references on rows with ONE product (the digits are integers before
the transform, so the only difference is the f64 rounding of that product), measured on the CPU mirrors (oracle modes 3
and 4, bit-identical to the kernels) over the committed row set:
    mode 3 (f64 FFT)          max |mirror - reference| = 2^23.70
    mode 4 (f64 FFT, two-bit) max |mirror - reference| = 2^24.58
T3 and T4 are 8 x those; a single wrong digit moves a coefficient by at least 2^41, more than 2^10 above either."""
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


def _product(desc, g, d):
    """Sparse external product of the digits d [2][2048] with GGSW g -> [2][2048]."""
    out = [np.zeros(N, U), np.zeros(N, U)]
    for col in range(2):
        for row in range(2):
            for coef, e in desc[(g, row, col)]:
                out[col] = out[col] + U(coef) * rot(d[row], e)
    return out


def _start(ms, lut):
    return [np.zeros(N, U), rot(np.asarray(lut, U), (2 * N - int(ms[LWE_N])) & (2 * N - 1))]


def blind_rotate_ref(desc, ms, lut, digit=digit, ties=None):
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
        p = _product(desc, i, [digit(x) for x in diff])
        acc = [acc[c] + p[c] for c in range(2)]
    return np.stack(acc)


def blind_rotate_mb2_ref(desc, ms, lut, digit=digit):
    """Two key bits per step: ACC += sum_t (X^e_t - 1) (K_t (.) ACC), t over (e1, e2, e1 + e2) -> [2, 2048]."""
    acc = _start(ms, lut)
    for p in range(LWE_N // 2):
        e1, e2 = int(ms[2 * p]), int(ms[2 * p + 1])
        if (e1 | e2) == 0:
            continue
        d = [digit(x) for x in acc]
        new = list(acc)
        for t, e in enumerate((e1, e2, (e1 + e2) & (2 * N - 1))):
            pt = _product(desc, 3 * p + t, d)
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
