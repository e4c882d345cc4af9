"""The ring Z_2^64[X]/(X^2048 + 1) in numpy with wrapping words and no transform: the schoolbook pieces that the host
tests of the packing tree and of the re-key family restate the library's formulas with (test_packed.py, test_rekey.py,
test_recipient.py, test_store_download.py, test_store.py).  Nothing here calls the library: being a second
implementation of the keyswitch arithmetic is the whole value of this file."""
import numpy as np

N = 2048
BIG_CT = 2049
U64 = np.uint64


def negacyclic(d, k):
    """sum_i d[i] X^i (*) k in Z_2^64[X]/(X^N + 1): d int64 (small), k uint64, schoolbook with wrapping words"""
    ext = np.concatenate([U64(0) - k, k])                        # ext[m] = +-k[m mod N]: the sign of X^N = -1
    rows = np.lib.stride_tricks.sliding_window_view(ext[1:], N)[:N, ::-1]   # rows[n][i] = ext[n - i + N]
    return (rows * d.astype(np.int64).view(U64)[None, :]).sum(axis=1, dtype=U64)


def digits(x, levels):
    """`levels` (2 or 3) signed 16-bit digits, most significant first, of the closest multiple of 2^(64 - 16 levels) to
    the uint64 words x: int64 arrays in [-2^15, 2^15); a carry out of the top digit is a multiple of 2^64"""
    assert levels in (2, 3)
    bits = 16 * levels
    v = ((x.astype(U64) + U64(1 << (63 - bits))) >> U64(64 - bits)) & U64((1 << bits) - 1)
    carry = np.zeros(v.shape, np.int64)
    out = [None] * levels
    for l in range(levels - 1, -1, -1):
        d = (v & U64(0xffff)).astype(np.int64) + carry
        v = v >> U64(16)
        carry = (d >= 1 << 15).astype(np.int64)
        out[l] = d - (carry << 16)
    return out


def digits32(a):
    """the two digits of a stored 32-bit word: a << 32 = d_0 2^48 + d_1 2^32 exactly"""
    return digits(a.astype(U64) << U64(32), 2)


def round32(x):
    return ((x + U64(1 << 31)) >> U64(32)).astype(np.uint32)


def round16(x):
    return ((x + U64(1 << 47)) >> U64(48)).astype(np.uint16)


def glwe_phases(mask, body, glwe_sk):
    """body - mask (*) S of every coefficient of one GLWE, uint64 words"""
    return body - negacyclic(glwe_sk.astype(np.int64), mask)


def packed_phases(p, glwe_sk):
    """body - mask (*) S of every block of a (windowed) packed string, words widened by << 48"""
    a_s = np.concatenate([glwe_phases(m.astype(U64) << U64(48), U64(0), glwe_sk) for m in p.mask16])
    return (p.body16.astype(U64) << U64(48)) + a_s[p.first_coef:p.first_coef + p.body16.size]


def block_phases(blocks, glwe_sk):
    """b - <a, s> of classic blocks [n][2049] under the big LWE key (the flattened GLWE key), wrapping uint64"""
    blocks = blocks.reshape(-1, BIG_CT)
    return blocks[:, N] - (blocks[:, :N] * glwe_sk[None, :]).sum(axis=1, dtype=U64)
