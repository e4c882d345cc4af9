"""The string store's GLWE keyswitch family -- the re-key in its three formats (DESIGN.md sections 14, 16, 17;
rekey_kernels.hip, rekey_host.cpp) and the select by encrypted index (section 23; select_kernels.hip, select_host.cpp)
-- restated in numpy with wrapping words, in the manner of pack_model.py: nothing here calls the library, and nothing
here multiplies polynomials through a transform.

Under a synthetic key the family is index arithmetic.  A re-key key or a query whose every polynomial is one word times
one monomial, `c X^e`, turns the term d_l (*) K into a signed roll of the digit polynomial times a word.  The identity
key (`identity_key`: mask rows -g_l X^m, body rows 0) returns X^m mask and the body itself; the noise-free GGSW of a bit
(`gadget_query`) makes a CMux exactly a + bit (b - a), so the select returns the words of the source row itself
(`selected_row`).  A key given as an array of words instead of a spec goes group by group (CMux by CMux) through the
schoolbook product.

`Rules` switches single formulas to a deliberately wrong variant: the negative controls of test_store_synth.py prove
with them that the chosen inputs tell a right kernel from a subtly wrong one.  `Tally` counts how often the inputs of a
run reach the boundaries they were chosen for."""
import dataclasses

import numpy as np

import pack_model as pm
from pack_model import grid, monomial_product
from ring_util import N, U64, negacyclic

GROUP = N
LEVELS = 2                                    # re-key digits; one CMux has 2 LEVELS digit polynomials
G0, G1 = 1 << 48, 1 << 32                     # the gadget: a << 32 = d_0 2^48 + d_1 2^32


@dataclasses.dataclass(frozen=True)
class Rules:
    """every field True: the formulas as DESIGN.md sections 14, 16, 17 and 23 state them"""
    rotate_wrap_negates: bool = True      # X^-s G: what wraps past X^N comes back negated
    stores_round: bool = True             # round32 / round16 add half before they shift
    tie_rounds_up: bool = True            # ... and a word exactly half way goes up
    low_carry_kept: bool = True           # a low digit >= 2^15 is negative and carries into the top digit
    top_carry_dropped: bool = True        # a top digit of 2^15 is -2^15: its carry is a multiple of 2^64
    key_on_grid: bool = True              # key and query are rounded to multiples of 2^6 first
    dead_sibling_is_zero: bool = True     # a node without a right sibling merges with zero, not with itself
    tree_bit_above_rotates: bool = True   # tree level t is steered by bit r + t, not by bit t
    absent_body_is_zero: bool = True      # body words past the last group's count are 0, not the neighbouring group's
    packed_mask_rounds_in: bool = True    # rekey_packed rounds its 64-bit mask to 32 bits, it does not shift


RIGHT = Rules()


# ---- the formulas ------------------------------------------------------------------------------------------------------
def _round(x, bits, rules):
    """the closest multiple of 2^bits to the uint64 words x, divided by it; ties upwards, the carry out of the top dropped
    (every word rounded here is a multiple of 2^6, so the last word below the tie is half - 64)"""
    half = 1 << (bits - 1)
    add = 0 if not rules.stores_round else half if rules.tie_rounds_up else half - 1
    return (np.asarray(x, U64) + U64(add)) >> U64(bits)


def round32(x, rules=RIGHT):
    return _round(x, 32, rules).astype(np.uint32)


def round16(x, rules=RIGHT):
    return _round(x, 48, rules).astype(np.uint16)


def digits2(w32, rules=RIGHT):
    """[d_0, d_1], int64 in [-2^15, 2^15), of the 32-bit words w: w << 32 = d_0 2^48 + d_1 2^32 modulo 2^64, exactly"""
    w = np.asarray(w32, np.uint32).astype(np.int64)
    lo, hi = w & 0xFFFF, w >> 16
    c1 = (lo >= 0x8000).astype(np.int64)
    d1 = lo - (c1 << 16)
    h = hi + (c1 if rules.low_carry_kept else 0)
    d0 = h - ((h >= 0x8000).astype(np.int64) << 16)
    if not rules.top_carry_dropped:
        d0 = np.where(h == 0x8000, 0x8000, d0)
    return [d0, d1]


def _is_dense(key):
    return isinstance(key, np.ndarray)


def keyswitch_sums(key, digs, rules=RIGHT):
    """(sum_l d_l (*) K[l].mask, sum_l d_l (*) K[l].body) for the digit polynomials digs[l] [..., N].  key: a spec,
    key[l][column] = (word, exponent) for the polynomial word X^exponent, or the words [len(digs)][2][N] themselves (any
    polynomials: the products are schoolbook sums, one leading index at a time)"""
    out = [np.zeros(digs[0].shape, U64), np.zeros(digs[0].shape, U64)]
    if _is_dense(key):
        K = (grid(key) if rules.key_on_grid else np.asarray(key, U64)).reshape(len(digs), 2, N)
        for l, d in enumerate(digs):
            assert int(d.min()) >= -(1 << 15) and int(d.max()) <= (1 << 15)
            for col in range(2):
                flat, acc = d.reshape(-1, N), out[col].reshape(-1, N)
                for i in range(len(flat)):
                    if flat[i].any():
                        acc[i] += negacyclic(flat[i], K[l, col])
        return out
    for l, d in enumerate(digs):
        for col in range(2):
            word, e = key[l][col]
            out[col] = out[col] + monomial_product(d, grid(word) if rules.key_on_grid else U64(word), e)
    return out


def _groups(n_blocks):
    return (n_blocks + GROUP - 1) // GROUP


def rekey(spec, mask32, body32, n_blocks, rules=RIGHT, tally=None):
    """the store's re-key (section 14): mask' = round32(-ks_mask), body' = round32((body << 32) - ks_body) -> (mask32
    [groups][N], body32 [n_blocks])"""
    g = _groups(n_blocks)
    mask = np.asarray(mask32, np.uint32).reshape(g, N)
    body = np.zeros(g * N, U64)
    body[:n_blocks] = np.asarray(body32, np.uint32).astype(U64) << U64(32)
    ks = keyswitch_sums(spec, digits2(mask, rules), rules)
    m, b = U64(0) - ks[0], (body.reshape(g, N) - ks[1]).reshape(-1)[:n_blocks]
    if tally is not None:
        tally.digit_words(mask)
        tally.stored("mask32", m, 32)
        tally.stored("body32", b, 32)
    return round32(m, rules), round32(b, rules)


def rekey_packed(spec, mask64, body64, n_blocks, rules=RIGHT, tally=None):
    """the packed download for a recipient (section 16): the mask rounded to 32 bits on the way in, the body at its 64
    bits, one rounding to 16 bits at the end -> (mask16 [groups][N], body16 [n_blocks])"""
    g = _groups(n_blocks)
    mask64 = np.asarray(mask64, U64).reshape(g, N)
    a = round32(mask64, rules) if rules.packed_mask_rounds_in else (mask64 >> U64(32)).astype(np.uint32)
    ks = keyswitch_sums(spec, digits2(a, rules), rules)
    m, b = U64(0) - ks[0], (np.asarray(body64, U64).reshape(g, N) - ks[1]).reshape(-1)[:n_blocks]
    if tally is not None:
        tally.stored("rekey_packed input mask", mask64, 32, below=False)
        tally.digit_words(a)
        tally.stored("mask16", m, 48)
        tally.stored("body16", b, 48)
    return round16(m, rules), round16(b, rules)


def store_packed(spec, mask32, body32, n_blocks, first_char, count, rules=RIGHT, tally=None):
    """the packed download of a parked entry (section 17), characters [first_char, first_char + count): the masks of the
    covering groups and the window's bodies -> (mask16 [covering groups][N], body16 [4 count], first_coef).  spec None:
    the own-key switch round16(w << 32)"""
    mask = np.asarray(mask32, np.uint32).reshape(_groups(n_blocks), N)
    t0, t1 = 4 * first_char, 4 * (first_char + count)
    g0, g1 = t0 // GROUP, (t1 - 1) // GROUP
    mask = mask[g0:g1 + 1]
    body = np.zeros((g1 + 1 - g0) * N, U64)
    have = min(n_blocks, (g1 + 1) * GROUP) - g0 * GROUP
    body[:have] = np.asarray(body32, np.uint32)[g0 * GROUP:g0 * GROUP + have].astype(U64) << U64(32)
    m = mask.astype(U64) << U64(32)
    if spec is not None:
        ks = keyswitch_sums(spec, digits2(mask, rules), rules)
        m, body = U64(0) - ks[0], (body.reshape(-1, N) - ks[1]).reshape(-1)
    b = body[t0 - g0 * GROUP:t1 - g0 * GROUP]
    if tally is not None and spec is not None:
        tally.digit_words(mask)
        tally.stored("mask16", m, 48)
        tally.stored("body16", b, 48)
    return round16(m, rules), round16(b, rules), t0 % GROUP


def rekey_key(spec):
    """the re-key key's words [level][mask, body][N] that spec[level][column] = (word, exponent) stands for, as they are
    loaded: the word itself, off the grid if it is"""
    key = np.zeros((len(spec), 2, N), U64)
    for l, row in enumerate(spec):
        for col in range(2):
            word, e = row[col]
            key[l, col, e] = U64(word)
    return key.reshape(-1)


def identity_key(m=0):
    """K[l] = (-g_l X^m, 0): the re-key under it returns mask' = X^m mask (negacyclic) and body' = body"""
    return [[((1 << 64) - G0, m), (0, 0)], [((1 << 64) - G1, m), (0, 0)]]


# ---- the select --------------------------------------------------------------------------------------------------------
def geometry(n_chars, row_chars):
    """(groups, row_blocks, rotate bits, tree levels) of DESIGN.md section 23"""
    rows, groups, row_blocks = n_chars // row_chars, _groups(4 * n_chars), 4 * row_chars
    bits = (rows - 1).bit_length()
    rot = bits if groups == 1 else (GROUP // row_blocks).bit_length() - 1
    return groups, row_blocks, rot, bits - rot


def cmux(rows, a, b, rules=RIGHT, tally=None):
    """out_col = round32((a_col << 32) + sum over the digit polynomials mask d_0, mask d_1, body d_0, body d_1 of D = b - a
    of d (*) rows[l].col); a, b, out = (mask32 [..., N], body32 [..., N]); rows: a spec [4][column] or words [4][2][N]"""
    digs = digits2(b[0] - a[0], rules) + digits2(b[1] - a[1], rules)
    ks = keyswitch_sums(rows, digs, rules)
    x = [(a[col].astype(U64) << U64(32)) + ks[col] for col in range(2)]
    if tally is not None:
        tally.digit_words(b[0] - a[0])
        tally.digit_words(b[1] - a[1])
        tally.stored("CMux mask32", x[0], 32)
        tally.stored("CMux body32", x[1], 32)
    return round32(x[0], rules), round32(x[1], rules)


def rotated(x, s, negate=True):
    """X^-s x along the last axis: coefficient n is x_(n + s), negated where n + s wraps"""
    out = np.roll(x, -s, axis=-1)
    if negate:
        out[..., N - s:] = np.uint32(0) - out[..., N - s:]
    return out


def _entry(mask32, body32, n_chars, rules):
    groups = _groups(4 * n_chars)
    body = np.zeros(groups * N, np.uint32)
    body[:4 * n_chars] = body32
    body = body.reshape(groups, N)
    count = 4 * n_chars - (groups - 1) * N
    if not rules.absent_body_is_zero and groups > 1:
        body[-1, count:] = body[-2, count:]
    return np.asarray(mask32, np.uint32).reshape(groups, N), body


def select(spec, mask32, body32, n_chars, row_chars, rules=RIGHT, tally=None):
    """the select in its fixed order: the tree over the groups first, level t under bit r + t with the zero GLWE for a
    missing right sibling, then G <- CMux(bit k, G, X^-(row_blocks << k) G) for the rotate bits -> (mask32 [N], body32
    [row_blocks]).  spec[bit] is what `cmux` takes as rows"""
    groups, row_blocks, rot, levels = geometry(n_chars, row_chars)
    m, b = _entry(mask32, body32, n_chars, rules)
    for t in range(levels):
        if len(m) & 1:
            pad = (m[-1:], b[-1:]) if not rules.dead_sibling_is_zero else (np.zeros((1, N), np.uint32),) * 2
            m, b = np.concatenate([m, pad[0]]), np.concatenate([b, pad[1]])
        bit = rot + t if rules.tree_bit_above_rotates else t
        m, b = cmux(spec[bit], (m[0::2], b[0::2]), (m[1::2], b[1::2]), rules, tally)
    m, b = m[0], b[0]
    for k in range(rot):
        s = row_blocks << k
        m, b = cmux(spec[k], (m, b), (rotated(m, s, rules.rotate_wrap_negates), rotated(b, s, rules.rotate_wrap_negates)),
                    rules, tally)
    return m, b[:row_blocks]


def query(spec):
    """the query's words [bits][4][mask, body][N] that spec[bit][row][column] = (word, exponent) stands for"""
    q = np.zeros((len(spec), 2 * LEVELS, 2, N), U64)
    for k, rows in enumerate(spec):
        for l in range(2 * LEVELS):
            for col in range(2):
                word, e = rows[l][col]
                q[k, l, col, e] = U64(word)
    return q


def gadget_bit(beta):
    """the noise-free GGSW of the bit beta, under any secret key: beta times the gadget matrix"""
    return [[(beta * G0, 0), (0, 0)], [(beta * G1, 0), (0, 0)], [(0, 0), (beta * G0, 0)], [(0, 0), (beta * G1, 0)]]


def gadget_query(index, bits):
    return [gadget_bit((index >> k) & 1) for k in range(bits)]


def selected_row(mask32, body32, n_chars, row_chars, index):
    """what a gadget query of `index` must return: group index >> r rolled left by row_blocks (index & (2^r - 1)), the
    sign flipped where it wraps; all zeros where the tree has no such group"""
    groups, row_blocks, rot, _ = geometry(n_chars, row_chars)
    m, b = _entry(mask32, body32, n_chars, RIGHT)
    grp, s = index >> rot, row_blocks * (index & ((1 << rot) - 1))
    if grp >= groups:
        return np.zeros(N, np.uint32), np.zeros(row_blocks, np.uint32)
    return rotated(m[grp], s), rotated(b[grp], s)[:row_blocks]


def names_a_row_or_a_missing_node(n_chars, row_chars, index):
    """False inside the unspecified tail of a partial last group (section 23, "an index p >= R")"""
    groups, _, rot, _ = geometry(n_chars, row_chars)
    return index < n_chars // row_chars or (index >> rot) >= groups


def true_sum(digs, polys, n):
    """coefficient n of sum_l d_l (*) K_l as a Python integer in grid units (K / 2^6, centred), no wrapping anywhere: what
    the exact transform has to hold"""
    total = 0
    for d, k in zip(digs, polys):
        kk = [int(v) >> 6 for v in grid(k)]
        kk = [v - (1 << 58) if v >= 1 << 57 else v for v in kk]
        dd = [int(v) for v in d]
        total += sum(dd[i] * kk[n - i] for i in range(n + 1)) - sum(dd[i] * kk[N + n - i] for i in range(n + 1, N))
    return total


# ---- how often a run's inputs reach the boundaries they were chosen for ---------------------------------------------------
def digit_classes(w32):
    """the two-digit carry chain of the 32-bit words w (pack_model.digit_classes without its third digit and its
    rounding: w << 32 is decomposed exactly), recomputed apart from digits2"""
    w = np.asarray(w32, np.uint32).astype(U64)
    d1 = w & U64(0xFFFF)
    c1 = d1 >= 0x8000
    d0 = (w >> U64(16)) + c1
    c0 = d0 >= 0x8000
    return {"digits: low digit 0x7FFF, the largest that does not carry": int((d1 == 0x7FFF).sum()),
            "digits: a digit of exactly -2^15": int((d1 == 0x8000).sum() + (d0 == 0x8000).sum()),
            "digits: carry of the low digit into the top": int(c1.sum()),
            "digits: ... and out of the top digit": int((c1 & c0).sum()),
            "digits: carry out of the top digit": int(c0.sum())}


def stored_classes(name, x, bits, below=True):
    """the rounding of the 64-bit words x to 64 - bits bits, as the array `name` stores them"""
    x = np.asarray(x, U64)
    low, half = x & U64((1 << bits) - 1), 1 << (bits - 1)
    out = {name + ": the tie, rounded up": int((low == half).sum())}
    if below:
        out[name + ": the last grid word below the tie, rounded down"] = int((low == half - 64).sum())
    out[name + ": rounded up past 2^64 to 0"] = int((x >= U64((1 << 64) - half)).sum())
    return out


class Tally(pm.Tally):
    """counts per boundary class over everything a run decomposes and stores"""

    def digit_words(self, x):
        self.add(digit_classes(x))
        self.counts["digits: words decomposed"] = self.counts.get("digits: words decomposed", 0) + int(np.asarray(x).size)

    def stored(self, name, x, bits, below=True):
        self.add(stored_classes(name, x, bits, below))


# ---- the chosen inputs that test_store_synth.py and test_store_synth_device.py share --------------------------------------
# mask words: the digit boundaries and the top carry (the six of the smoke run), then single digits of +-1 and 3, whose
# product with a key word is the key word itself
MASK_WORDS = np.array((0x00000000, 0x00008000, 0x7FFF8000, 0x80000000, 0xFFFFFFFF, 0x00007FFF,
                       1, 0x00010000, 0xFFFF0000, 3), np.uint32)
BODY_WORDS = np.array((0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF), np.uint32)
BODY64_WORDS = np.array((0, (1 << 64) - (1 << 48), 1 << 63, 1 << 47), U64)
# low halves of a 64-bit mask word: both sides of the input rounding's tie, and the ends
MASK64_LOW = np.array((0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x7FFFFFC0), U64)
# key words that put d c on the boundaries of round32 (2^31) and round16 (2^47) for a digit d of +-1, 2^63, and the
# off-grid and extreme words of the packing tree's tests
BOUNDARY_KEY_WORDS = (1 << 31, (1 << 31) - 64, (1 << 31) + 64, 1 << 47, (1 << 47) - 64, (1 << 47) + 64, 1 << 63)
KEY_WORDS = BOUNDARY_KEY_WORDS + pm.KEY_WORDS
EXPONENTS = (0, 1, 1024, 2047)
EXTREME_KEY_WORD = 0x7FFFFFFFFFFFFFC0         # the largest grid word: 2^57 - 1 grid units
EXTREME_WORD = 0x7FFF8000                     # both digits -2^15
BLOCK_COUNTS = (1, 24, 2048, 2052, 5 * 2048 + 3)
WINDOW_CHARS = (513, 1026, 2561)
SHAPES = ((2, 1), (512, 1), (1024, 512), (1536, 512), (640, 128), (2624, 64))     # (n_chars, row_chars)
MONOMIAL_SHAPES = ((2, 1), (512, 1), (1536, 512), (2624, 64))


def windows(n):
    """(first_char, count): the window shapes of the smoke run's packed download of parked entries"""
    w = [(0, n), (0, 1), (511, 1), (511, 2), (512, 1), (512, 512), (n - 1, 1)] + ([(511, 514)] if n == 1026 else [])
    return [x for x in w if x[0] + x[1] <= n]


def chosen(rng, shape, words):
    """about two in three words from `words`, the rest random"""
    words = np.asarray(words)
    out = rng.integers(0, 1 << (8 * words.dtype.itemsize), shape, dtype=words.dtype)
    pick = rng.random(shape) < 2 / 3
    out[pick] = rng.choice(words, int(pick.sum()))
    return out


def chosen_mask64(rng, shape):
    """64-bit mask words whose round32 is a word of `chosen(.., MASK_WORDS)`: low halves on both sides of the tie"""
    want = chosen(rng, shape, MASK_WORDS).astype(U64)
    low = chosen(rng, shape, MASK64_LOW) & U64(0xFFFFFFFF)
    return ((want - (low >> U64(31))) << U64(32)) | low


def rekey_words(n_blocks, seed=0):
    """(mask32 [groups][N], body32 [n_blocks]) of chosen words for a raw re-key"""
    rng = np.random.default_rng(7000 + 31 * seed + n_blocks)
    return chosen(rng, (_groups(n_blocks), N), MASK_WORDS), chosen(rng, n_blocks, BODY_WORDS)


def packed_words(n_blocks, seed=0):
    """(mask64, body64) [groups][N] of chosen words for rekey_packed"""
    rng = np.random.default_rng(8000 + 31 * seed + n_blocks)
    return chosen_mask64(rng, (_groups(n_blocks), N)), chosen(rng, (_groups(n_blocks), N), BODY64_WORDS)


def entry_words(n_chars, seed=0):
    """(mask32 [groups][N], body32 [4 n_chars]) of chosen words for an entry of whole characters"""
    return rekey_words(4 * n_chars, seed + 1)


A_KEY, B_KEY = "2^47, 2^31 and 2^31 + 64", "2^47 +- 64 and 2^31 - 64"
OFF32_KEY, OFF16_KEY = "off the grid next to 2^31", "off the grid next to 2^47"


def rekey_specs():
    """re-key keys of monomials, spec[level][column] = (word, exponent): every key word above between them, every
    exponent of EXPONENTS in each.  In the first two the other level's word of a column is 2^63 or a gadget word, whose
    products vanish below 2^32, so that one product alone decides a stored word's low bits.  In the next two a word off
    the grid (0x1F rounds to 0, 0x20 to 0x40) meets one that puts odd digits on the tie of round32 or round16: 32 d more
    or less decides which way the stored word goes.  The rest walk through the remaining words"""
    specs = {A_KEY: [[(1 << 47, 1024), (1 << 31, 2047)], [(1 << 63, 0), ((1 << 31) + 64, 1)]],
             B_KEY: [[((1 << 47) - 64, 1), ((1 << 47) + 64, 0)], [((1 << 31) - 64, 1024), ((1 << 64) - G1, 2047)]],
             OFF32_KEY: [[(0x1F, 1), (0x20, 0)], [(1 << 31, 1024), ((1 << 31) + 64, 2047)]],
             OFF16_KEY: [[(0x1F, 0), (0x20, 1024)], [(1 << 47, 2047), ((1 << 47) + 64, 1)]]}
    rest = [w for w in KEY_WORDS if w not in [x for s in specs.values() for row in s for x, _ in row]]
    rest += list(BOUNDARY_KEY_WORDS[:(-len(rest)) % 4])
    for k in range(len(rest) // 4):
        w = rest[4 * k:4 * k + 4]
        specs["key words %d.." % (4 * k)] = [[(w[2 * l + col], EXPONENTS[(k + 2 * l + col) % 4]) for col in range(2)]
                                             for l in range(LEVELS)]
    return specs


A_QUERY, B_QUERY = "boundary words first", "extreme words first"
# words whose product with any digit vanishes below 2^32 once the word is on the grid (0x1F and 0xFF..E0 round to 0,
# 0x7FF..E0 to 2^63): next to them one other word alone decides a stored word's low bits
_QUIET = (1 << 63, 0xFFFFFFFFFFFFFFE0, 1 << 47, 0x7FFFFFFFFFFFFFE0)


def select_specs(bits):
    """two queries of monomials for `bits` index bits, spec[bit][row][column] = (word, exponent).  Every third bit is the
    gadget of a set bit (from bit 0 in the first query, from bit 1 in the second).  Every other bit takes the next two of
    KEY_WORDS, in that order or with the extreme words first, one per column in rows that move from bit to bit; the
    column's other rows hold 0x1F and two quiet words.  A query of one bit keeps the gadget in half of its rows instead,
    the body digits' in the first query and the mask digits' in the second: all gadget, it would be a gadget query"""
    out = {}
    # 2^31 in the body column of the second bit; the two queries of six or more bits hold every key word between them
    extreme_first = pm.KEY_WORDS[:3] + BOUNDARY_KEY_WORDS[:1] + pm.KEY_WORDS[5:] + BOUNDARY_KEY_WORDS[1:] + pm.KEY_WORDS[3:5]
    for name, words, phase in ((A_QUERY, KEY_WORDS, 0), (B_QUERY, extreme_first, 1)):
        spec, j = [], 0
        for k in range(bits):
            if bits > 1 and k % 3 == phase:
                spec.append(gadget_bit(1))
                continue
            rows = [[None, None] for _ in range(2 * LEVELS)]
            for col in range(2):
                at = (j + 2 * col) % 4
                rows[at][col] = (words[(2 * j + col) % len(words)], EXPONENTS[(j + col) % 4])
                for i, l in enumerate(x for x in range(4) if x != at):
                    rows[l][col] = (0x1F if i == 0 else _QUIET[(j + col + i) % 4], EXPONENTS[(j + col + i + 1) % 4])
            if bits == 1:
                keep = slice(2, 4) if phase == 0 else slice(0, 2)
                rows[keep] = gadget_bit(1)[keep]
            spec.append(rows)
            j += 1
        out[name] = spec
    return out
