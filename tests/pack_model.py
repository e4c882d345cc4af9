"""The packing tree of the packed download (pack_kernels.hip, pack_host.cpp) restated in numpy with
wrapping words, in the manner of ring_util.py: nothing here calls the library, and nothing here multiplies polynomials
through a transform.

Under a synthetic packing key the tree is index arithmetic.  With the zero key every keyswitch sum vanishes and the
result has a closed form (`zero_key_pack`); with a key whose every polynomial is one word times one monomial, `c X^m`,
the term d_l (*) K is a signed roll of the digit polynomial times a word, and the tree is a recursion on 2048-vectors
(`tree`).  A dense key goes node by node through the schoolbook product (`node_dense`).

`Rules` switches single formulas to a deliberately wrong variant: the negative controls of test_pack_synth.py prove
with them that the chosen inputs tell a right tree from a subtly wrong one.  `Tally` counts how often the inputs of a
run reach the boundaries they were chosen for."""
import dataclasses

import numpy as np

from ring_util import N, U64, digits, negacyclic, round16, round32  # noqa: F401  (round16 / round32: part of the model)

BIG_CT = 2049
LEVELS, TREE_LEVELS, GROUP = 3, 11, 2048
DELTA_LOG = 59


@dataclasses.dataclass(frozen=True)
class Rules:
    """every field True: the tree as DESIGN.md section 11 states it"""
    shift_wrap_negates: bool = True       # X^t O: what wraps past X^N comes back negated
    automorphism_signed: bool = True      # coefficient i of A lands at i g mod N with the sign of X^N = -1
    prescale_rounds: bool = True          # (x + 2^10) >> 11, not x >> 11
    digits_round: bool = True             # digits of the closest multiple of 2^16, not of the floor
    key_on_grid: bool = True              # the key is rounded to multiples of 2^6 first
    dead_odd_is_zero: bool = True         # a node without an odd child merges with zero, not with its even child again


RIGHT = Rules()


# ---- the formulas ------------------------------------------------------------------------------------------------------
def prescale(x, rules=RIGHT):
    """division by N = 2^11 with rounding (ties upwards); the add wraps at 2^64 - 2^10"""
    return (x + U64(1 << 10 if rules.prescale_rounds else 0)) >> U64(11)


def leaf(block, rules=RIGHT):
    """the leaf GLWE [..., 2, N] of classic blocks [..., 2049]: A_0 = a_0, A_{N-i} = -a_i, B_0 = b, all pre-scaled"""
    pre = prescale(block, rules)
    out = np.zeros(block.shape[:-1] + (2, N), U64)
    out[..., 0, 0] = pre[..., 0]
    out[..., 0, 1:] = (U64(0) - pre[..., 1:N])[..., ::-1]
    out[..., 1, 0] = pre[..., N]
    return out


def trivial_char(v):
    """the four blocks [4][2049] of a trivial character: zero masks, two message bits per block at 2^59, low bits first"""
    out = np.zeros((4, BIG_CT), U64)
    out[:, N] = [((int(v) >> (2 * b)) & 3) << DELTA_LOG for b in range(4)]
    return out


def grid(k):
    """the closest multiple of 2^6 (ties upwards, modulo 2^64): the 58-bit grid every keyswitch key is loaded on"""
    return (np.asarray(k, U64) + U64(32)) & ~U64(63)


def automorphism(a, g, rules=RIGHT):
    """A(X^g) along the last axis, by index: coefficient i goes to i g mod N, negated when i g mod 2N >= N"""
    idx = (np.arange(N, dtype=np.int64) * g) % (2 * N)
    out = np.zeros_like(a)
    out[..., idx % N] = np.where(idx >= N, U64(0) - a, a) if rules.automorphism_signed else a
    return out


def shift(a, m, negate=True):
    """X^m A along the last axis, 0 <= m < N"""
    if m == 0:
        return a.copy()
    head = a[..., N - m:]
    return np.concatenate([U64(0) - head if negate else head, a[..., :N - m]], axis=-1)


def monomial_product(d, word, m):
    """d (*) word X^m for a digit polynomial d (int64, small) and one torus word: roll plus sign, wrapping uint64"""
    return shift(d.astype(np.int64).view(U64) * U64(word), m)


def _digits(a, rules):
    return digits(a if rules.digits_round else a - U64(1 << 15), LEVELS)     # (ring_util.digits adds 2^15 itself)


def merge(lv, e, o, rules):
    """P = E + X^t O, and the two polynomials of (E - X^t O)(X^g); e, o [..., 2, N]"""
    t, g = N >> lv, (1 << lv) + 1
    T = shift(o, t, rules.shift_wrap_negates)
    P, M = e + T, e - T
    return P, automorphism(M[..., 0, :], g, rules), automorphism(M[..., 1, :], g, rules)


def node(level_key, lv, e, o, rules=RIGHT, tally=None):
    """out = P + AutoKS_g(M) of one tree level's nodes [..., 2, N] under a monomial key: level_key[digit][column] =
    (word, exponent) stands for the key polynomial word X^exponent"""
    P, a1, b1 = merge(lv, e, o, rules)
    if tally is not None:
        tally.digit_words(a1)
    dig = _digits(a1, rules)
    s = [np.zeros_like(a1), np.zeros_like(a1)]
    for l in range(LEVELS):
        for col in range(2):
            word, m = level_key[l][col]
            s[col] = s[col] + monomial_product(dig[l], grid(word) if rules.key_on_grid else U64(word), m)
    return np.stack([P[..., 0, :] - s[0], P[..., 1, :] + b1 - s[1]], axis=-2)


def node_dense(key, lv, e, o):
    """the same node, one at a time, under a dense key of [11][LEVELS][2][N] words (off the grid or on it): the
    negacyclic products are schoolbook sums"""
    kg = grid(key).reshape(TREE_LEVELS, LEVELS, 2, N)[lv - 1]
    P, a1, b1 = merge(lv, e, o, RIGHT)
    dig = digits(a1, LEVELS)
    assert all(int(d.min()) >= -(1 << 15) and int(d.max()) < (1 << 15) for d in dig)
    sm, sb = np.zeros(N, U64), np.zeros(N, U64)
    for l in range(LEVELS):
        sm += negacyclic(dig[l], kg[l, 0])
        sb += negacyclic(dig[l], kg[l, 1])
    return np.stack([P[0] - sm, P[1] + b1 - sb])


def monomial_key(spec):
    """the key words [11 * LEVELS * 2 * N] that spec[level][digit][column] = (word, exponent) stands for, as they are
    loaded: the word itself, off the grid if it is"""
    key = np.zeros((TREE_LEVELS, LEVELS, 2, N), U64)
    for lv in range(TREE_LEVELS):
        for l in range(LEVELS):
            for col in range(2):
                word, m = spec[lv][l][col]
                key[lv, l, col, m] = U64(word)
    return key.reshape(-1)


def tree(spec, blocks, rules=RIGHT, tally=None, chunk=256):
    """blocks [n][2049] -> (mask64, body64) [groups][N] under the monomial key `spec`.  Groups are 2048 blocks.  Node k of
    level lv is live if k < min(count, 2048 >> lv); its children are nodes k (even) and k + (2048 >> lv) (odd) of the
    level below, the blocks themselves below level 1; the odd child is live if k + (2048 >> lv) < count."""
    blocks = blocks.reshape(-1, BIG_CT)
    groups = (len(blocks) + GROUP - 1) // GROUP
    mask, body = np.zeros((groups, N), U64), np.zeros((groups, N), U64)
    for grp in range(groups):
        mine = blocks[grp * GROUP:(grp + 1) * GROUP]
        count = len(mine)
        if tally is not None:
            tally.prescale_words(mine)
        cur = leaf(mine, rules)
        for lv in range(1, TREE_LEVELS + 1):
            n_lv = N >> lv
            live = min(count, n_lv)
            n_odd = max(0, min(count - n_lv, live))
            nxt = np.empty((live, 2, N), U64)
            for k0 in range(0, live, chunk):                       # (a level of 1024 nodes at once would want gigabytes)
                k1 = min(live, k0 + chunk)
                e = cur[k0:k1]
                o = np.zeros_like(e) if rules.dead_odd_is_zero else e.copy()
                if k0 < n_odd:
                    o[:min(k1, n_odd) - k0] = cur[n_lv + k0:n_lv + min(k1, n_odd)]
                nxt[k0:k1] = node(spec[lv - 1], lv, e, o, rules, tally)
            cur = nxt
        mask[grp], body[grp] = cur[0, 0], cur[0, 1]
    return mask, body


_ZERO_KEY_INDEX = []


def zero_key_pack(blocks):
    """what the tree leaves under the all-zero key, in closed form: body coefficient j = 2048 prescale(b_j) for
    j < count and 0 beyond; mask = sum_j X^j leaf_j, that is mask[n] = sum_{j >= n} p(a_j[j - n]) - sum_{j < n} p(a_j[N + j - n])"""
    blocks = blocks.reshape(-1, BIG_CT)
    groups = (len(blocks) + GROUP - 1) // GROUP
    mask, body = np.zeros((groups, N), U64), np.zeros((groups, N), U64)
    if not _ZERO_KEY_INDEX:
        j, n = np.arange(N)[:, None], np.arange(N)[None, :]
        _ZERO_KEY_INDEX.extend([(j - n) % N, j < n])
    col, negative = _ZERO_KEY_INDEX
    for grp in range(groups):
        mine = prescale(blocks[grp * GROUP:(grp + 1) * GROUP])
        count = len(mine)
        body[grp, :count] = mine[:, N] * U64(N)
        terms = np.take_along_axis(mine[:, :N], col[:count], axis=1)
        mask[grp] = np.where(negative[:count], U64(0) - terms, terms).sum(axis=0, dtype=U64)
    return mask, body


# ---- how often a run's inputs reach the boundaries they were chosen for ---------------------------------------------------
def prescale_classes(x):
    low = np.asarray(x, U64) & U64(0x7FF)
    return {"prescale: low bits 0x3FF, the last word rounded down": int((low == 0x3FF).sum()),
            "prescale: low bits 0x400, the tie, rounded up": int((low == 0x400).sum()),
            "prescale: the add wraps at 2^64 - 2^10": int((np.asarray(x, U64) >= U64(0xFFFFFFFFFFFFFC00)).sum())}


def digit_classes(x):
    """the three-digit carry chain of the words x, recomputed apart from ring_util.digits"""
    x = np.asarray(x, U64)
    v = ((x + U64(1 << 15)) >> U64(16)) & U64((1 << 48) - 1)
    d2 = v & U64(0xFFFF)
    c2 = d2 >= 0x8000
    d1 = ((v >> U64(16)) & U64(0xFFFF)) + c2
    c1 = d1 >= 0x8000
    d0 = (v >> U64(32)) + c1
    c0 = d0 >= 0x8000
    return {"digits: low 16 bits 0x7FFF, the last word rounded down": int(((x & U64(0xFFFF)) == 0x7FFF).sum()),
            "digits: low 16 bits 0x8000, the tie, rounded up": int(((x & U64(0xFFFF)) == 0x8000).sum()),
            "digits: the rounding add wraps at 2^64 - 2^15": int((x >= U64(0xFFFFFFFFFFFF8000)).sum()),
            "digits: a digit of exactly -2^15": int(((d2 == 0x8000).sum() + (d1 == 0x8000).sum() + (d0 == 0x8000).sum())),
            "digits: carry of the low digit through the middle one into the top": int((c2 & c1).sum()),
            "digits: ... and out of the top digit": int((c2 & c1 & c0).sum()),
            "digits: carry out of the top digit": int(c0.sum())}


def round_classes(x, bits):
    """round16 (bits = 48) / round32 (bits = 32) of the words x"""
    x = np.asarray(x, U64)
    low, half, name = x & U64((1 << bits) - 1), 1 << (bits - 1), "round%d" % (64 - bits)
    return {name + ": low bits one below the tie, rounded down": int((low == half - 1).sum()),
            name + ": the tie, rounded up": int((low == half).sum()),
            name + ": rounded up past 2^64 to 0": int((x >= U64((1 << 64) - half)).sum())}


def key_classes(words):
    w = np.asarray(words, U64)
    return {"key: off the 2^6 grid": int(((w & U64(63)) != 0).sum()),
            "key: the tie 0x20, rounded up": int(((w & U64(63)) == 32).sum()),
            "key: rounds to 2^63": int(((grid(w) == U64(1 << 63)) & (w != U64(1 << 63))).sum()),
            "key: rounds past 2^64 to 0": int((w >= U64(0xFFFFFFFFFFFFFFE0)).sum())}


class Tally:
    """counts per boundary class over everything a run of `tree` pre-scales and decomposes"""

    def __init__(self):
        self.counts = {}

    def add(self, classes):
        for name, n in classes.items():
            self.counts[name] = self.counts.get(name, 0) + n

    def prescale_words(self, x):
        self.add(prescale_classes(x))

    def digit_words(self, x):
        self.add(digit_classes(x))
        self.counts["digits: words decomposed"] = self.counts.get("digits: words decomposed", 0) + int(np.asarray(x).size)

    def __str__(self):
        return "\n".join("    %-72s %d" % (k, v) for k, v in self.counts.items())


# ---- the chosen inputs that test_pack_synth.py and test_pack_synth_device.py share ----------------------------------------
# key words: 2^63; the largest grid word below it; off the grid on both sides of the tie; one that rounds past 2^64 to 0;
# one that rounds to 2^63; and ordinary grid words
KEY_WORDS = (0x8000000000000000, 0x7FFFFFFFFFFFFFC0, 0x1F, 0x20, 0xFFFFFFFFFFFFFFE0, 0x7FFFFFFFFFFFFFE0,
             0x0123456789ABCDC0, 0x40, 0xFEDCBA9876543200, 0x8000000000000040)
# prescaled values p on the digit boundaries; a block word p << 11 becomes +p in a leaf's coefficient 0 and in its
# body, -p elsewhere, and the automorphism's signs turn half of those round again
_DIGIT_P = (0x7FFF, 0x8000, 0x7FFFFFFF8000, 0x7FFF7FFF8000, 0x800080008000, 0x7FFF80000000, 0x800080000000, 0x7FFF7FFF7FFF)
# round16 of a packed word under the zero key: bodies b with 2048 prescale(b) on both sides of 2^47 and of the wrap to 0,
# and mask words a with +-prescale(a) = +-2^47 and one beyond
ROUND16_BODY_WORDS = (0x00007FFFFFFFFBFF, 0x00007FFFFFFFFC00, 0xFFFF7FFFFFFFFBFF, 0xFFFF7FFFFFFFFC00)
ROUND16_MASK_WORDS = (0x7FFFFFFFFFFF << 11, 1 << 58, (1 << 58) + 2048)
BLOCK_WORDS = np.array(
    (0x3FF, 0x400, 0xBFF, 0xC00, 0xFFFFFFFFFFFFFBFF, 0xFFFFFFFFFFFFFC00,         # the prescale's rounding and its wrap
     0, 1 << 63, (1 << 63) - 1) +
    tuple(p << 11 for p in _DIGIT_P) + ROUND16_BODY_WORDS + ROUND16_MASK_WORDS, np.uint64)
# the three-digit boundary words of a node's inputs
NODE_WORDS = np.array((0x7FFF, 0x8000, 0x00007FFFFFFF8000, 0x7FFF7FFF7FFF8000, 0x7FFFFFFFFFFF8000, 0xFFFFFFFFFFFF8000,
                       1 << 63, 0x7FFF800000000000, 0, (1 << 64) - 1), np.uint64)


def monomial_specs():
    """two keys of monomials, spec[level][digit][column] = (word, exponent): every key word above, exponents that
    include 0 and 2047"""
    rng = np.random.default_rng(2)
    a = [[[(KEY_WORDS[(3 * lv + 2 * l + col) % len(KEY_WORDS)], int(rng.integers(0, N))) for col in range(2)]
          for l in range(LEVELS)] for lv in range(TREE_LEVELS)]
    a[0][0][0] = (KEY_WORDS[0], 0)
    a[10][2][1] = (KEY_WORDS[1], N - 1)
    b = [[[(KEY_WORDS[(7 * lv + 3 * l + 5 * col + 1) % len(KEY_WORDS)], (0, N - 1, 1, N // 2)[(lv + l + col) % 4]) for col in range(2)]
          for l in range(LEVELS)] for lv in range(TREE_LEVELS)]
    return {"scattered exponents": a, "exponents 0, 2047, 1 and 1024": b}


def chosen_blocks(rng, n, trivial=()):
    """n blocks [n][2049]: six in ten of all words, masks and bodies, from BLOCK_WORDS, the rest random; the blocks listed in
    `trivial` with an all-zero mask"""
    blocks = rng.integers(0, 1 << 64, (n, BIG_CT), dtype=np.uint64)
    pick = rng.random((n, BIG_CT)) < 0.6
    blocks[pick] = rng.choice(BLOCK_WORDS, int(pick.sum()))
    for k in trivial:
        blocks[k, :N] = 0
    return blocks
