"""Packed result download under a recipient's key, on the host (include/fhestring_hip.h, "packed result download under a
recipient's key"): fhs_rekey_packed_host against a numpy restatement of the formulas that uses no
transform, block counts of every kind, the real flow a -> b with the noise against an own-key download of the same
GLWEs, and the ABI edges.  The device kernel is compared with the host reference, word for word, in smoke() of
__graft_entry__.py (tests/test_recipient_device.py runs that step alone)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from ring_util import digits32, negacyclic, packed_phases, round16

N = 2048
LEVELS = 2
FHS_ERR_STATE = -3
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 64-bit mask words on the input-rounding and digit boundaries -> the 32-bit word a = (M + 2^31) >> 32 they must give
BOUNDARY = ((0x000000007FFFFFFF, 0x00000000), (0x0000000080000000, 0x00000001), (0x00007FFF7FFFFFFF, 0x00007FFF),
            (0x00007FFF80000000, 0x00008000), (0x7FFF7FFF80000000, 0x7FFF8000), (0xFFFFFFFF80000000, 0x00000000),
            (0x8000000000000000, 0x80000000), (0xFFFFFFFF7FFFFFFF, 0xFFFFFFFF))
SENTINEL = 0xA5A5


def _np_group(key, mask64, body64, count):
    """the formulas of one group"""
    K = ((key + U64(32)) & ~U64(63)).reshape(LEVELS, 2, N)        # round_to_grid(., 6)
    a = ((mask64 + U64(1 << 31)) >> U64(32)).astype(np.uint32)    # wraps at the top
    d = digits32(a)
    A = a.astype(U64) << U64(32)
    assert np.array_equal(d[0].view(U64) << U64(48), A - (d[1].view(U64) << U64(32)))         # A = d_0 2^48 + d_1 2^32
    assert all(int(x.min()) >= -(1 << 15) and int(x.max()) < (1 << 15) for x in d)
    s = [sum((negacyclic(d[l], K[l, col]) for l in range(LEVELS)), np.zeros(N, U64)) for col in range(2)]
    return a, round16(U64(0) - s[0]), round16(body64[:count] - s[1][:count])


@pytest.fixture(scope="module")
def flow():
    """Clients a and b from the fixed seeds; a 513-character string (two groups, the second with 4 blocks) encrypted by a
    as blocks, packed with a's packing key on the host, and switched to b's key: computed once for the tests below."""
    from fhestring_amd.api import MyClientKey, pack_host, rekey_packed_host
    a, b = MyClientKey(0x5EEDA), MyClientKey(0x5EEDB)
    text = "".join(chr(33 + (7 * i) % 90) for i in range(513))
    m64, b64 = pack_host(a.packing_key(), a.encrypt_str_raw(text, 0))
    m64.setflags(write=False)
    b64.setflags(write=False)
    p = rekey_packed_host(a.rekey_key(b), m64, b64, 4 * 513)
    yield a, b, text, m64, b64, p
    a.close()
    b.close()


def test_host_reference_equals_schoolbook_in_every_word():
    from fhestring_amd.api import REKEY_KEY_WORDS, rekey_packed_host
    rng = np.random.default_rng(16)
    key = rng.integers(0, 1 << 64, REKEY_KEY_WORDS, dtype=U64)     # off the grid: the reference rounds it first
    mask = rng.integers(0, 1 << 64, (1, N), dtype=U64)
    body = rng.integers(0, 1 << 64, (1, N), dtype=U64)
    _, wm, wb = _np_group(key, mask[0], body[0], N)
    got = rekey_packed_host(key, mask, body, N)
    assert np.array_equal(got.mask16[0], wm) and np.array_equal(got.body16, wb)
    # the boundary words, all of them in one polynomial: each one at its first positions, then drawn at random
    words = np.array([w for w, _ in BOUNDARY], U64)
    mask = rng.choice(words, (1, N))
    mask[0, :len(words)] = words
    a, wm, wb = _np_group(key, mask[0], body[0], N)
    assert [int(x) for x in a[:len(words)]] == [want for _, want in BOUNDARY]
    assert int(digits32(a[3:4])[1][0]) == -0x8000 and int(digits32(a[3:4])[0][0]) == 1           # the low digit turns negative
    got = rekey_packed_host(key, mask, body, N)
    assert np.array_equal(got.mask16[0], wm) and np.array_equal(got.body16, wb)
    # ... and each of them alone, throughout a mask, with fewer bodies than coefficients
    for w, _ in BOUNDARY:
        mask = np.full((1, N), w, U64)
        _, wm, wb = _np_group(key, mask[0], body[0], 777)
        gm, gb = rekey_packed_host(key, mask, body, 777)
        assert np.array_equal(gm[0], wm) and np.array_equal(gb, wb), hex(w)


def test_block_counts_of_every_kind():
    import fhestring_amd
    from fhestring_amd.api import REKEY_KEY_WORDS
    L = fhestring_amd.lib()
    rng = np.random.default_rng(17)
    key = rng.integers(0, 1 << 64, REKEY_KEY_WORDS, dtype=U64)
    for n_blocks in (1, 24, 2048, 2052, 5 * N + 3):
        g = (n_blocks + N - 1) // N
        mask = rng.integers(0, 1 << 64, (g, N), dtype=U64)
        body = rng.integers(0, 1 << 64, (g, N), dtype=U64)
        m16 = np.full((g, N), SENTINEL, np.uint16)
        b16 = np.full((g, N), SENTINEL, np.uint16)                 # room for whole groups: what lies beyond stays
        assert L.fhs_rekey_packed_host(key.ctypes.data, mask.ctypes.data, body.ctypes.data, n_blocks, m16.ctypes.data,
                                       b16.ctypes.data) == 0
        flat = b16.reshape(-1)
        assert (flat[n_blocks:] == SENTINEL).all(), n_blocks
        for k in range(g):                                         # every group equals the reference on that group alone
            count = min(N, n_blocks - k * N)
            m1, b1 = np.full(N, SENTINEL, np.uint16), np.full(N, SENTINEL, np.uint16)
            assert L.fhs_rekey_packed_host(key.ctypes.data, mask[k].ctypes.data, body[k].ctypes.data, count, m1.ctypes.data,
                                           b1.ctypes.data) == 0
            assert np.array_equal(m16[k], m1) and np.array_equal(flat[k * N:k * N + count], b1[:count]), (n_blocks, k)
            assert (b1[count:] == SENTINEL).all()
        if n_blocks <= 24:                                         # ... and the formulas, where one product is enough
            _, wm, wb = _np_group(key, mask[0], body[0], n_blocks)
            assert np.array_equal(m16[0], wm) and np.array_equal(flat[:n_blocks], wb)


def test_it_decrypts_under_the_recipients_key(flow):
    a, b, text, m64, b64, p = flow
    assert len(p) == 513 and p.mask16.shape == (2, N) and p.body16.shape == (2052,)
    assert b.decrypt_packed(p) == text
    want = np.array([(ord(ch) >> (2 * k)) & 3 for ch in text for k in range(4)], np.uint8)
    assert np.array_equal(b.decrypt_packed_blocks(p), want)
    try:
        wrong = a.decrypt_packed(p)
    except UnicodeDecodeError:                                       # not even ASCII
        wrong = None
    assert wrong != text
    assert not np.array_equal(a.decrypt_packed_blocks(p), want)


def test_noise_against_an_own_key_download(flow):
    """The recipient's phase error against an own-key download of the same 64-bit GLWEs: both are dominated by the 16-bit
    rounding, 2^48 sqrt((1 + |S|^2) / 12) ~ 2^51.2, under keys of equal weight, so the own-key sigma measured here is the
    reference (factor 2); decoding fails at 2^58, and 2^55 is about 14 sigma of the derived figure."""
    from fhestring_amd.api import pack_switch16
    a, b, text, m64, b64, p = flow
    n_blocks = 4 * len(text)
    want = np.array([(ord(ch) >> (2 * k)) & 3 for ch in text for k in range(4)], U64) << U64(59)
    sa, sb = a.secret_keys()[1], b.secret_keys()[1]
    own = pack_switch16(m64, b64, n_blocks)
    e_own = (packed_phases(own, sa) - want).view(np.int64).astype(np.float64)
    e_rec = (packed_phases(p, sb) - want).view(np.int64).astype(np.float64)
    s_own, s_rec = float(e_own.std()), float(e_rec.std())
    derived = 2.0 ** 48 * math.sqrt((1 + float(sb.sum())) / 12)
    print("recipient download: sigma 2^%.2f, own-key sigma 2^%.2f, derived 2^%.2f, max |e| 2^%.2f (own key 2^%.2f)" %
          (math.log2(s_rec), math.log2(s_own), math.log2(derived), math.log2(np.abs(e_rec).max()),
           math.log2(np.abs(e_own).max())))
    assert s_own / 2 < s_rec < s_own * 2
    assert np.abs(e_rec).max() < 2.0 ** 55


def test_abi_edges():
    import fhestring_amd
    from fhestring_amd.api import FhsError, MyServerKey, PackedFheString, REKEY_KEY_WORDS, _harr
    L = fhestring_amd.lib()
    sk = MyServerKey.planner()
    try:
        sk.load_rekey_key(np.zeros(REKEY_KEY_WORDS, U64))
        s = sk.dummy_string(3)
        with pytest.raises(FhsError) as e:
            sk.download_packed(s, recipient=True)
        assert e.value.code == FHS_ERR_STATE and "planner" in str(e.value)
        with pytest.raises(FhsError) as e:
            sk.download_packed(s, wide=True, recipient=True)
        assert e.value.code == FHS_ERR_STATE
        with pytest.raises(FhsError) as e:
            sk.ctx.rekey_packed_device(np.zeros((1, N), U64), np.zeros((1, N), U64), 5)
        assert e.value.code == FHS_ERR_STATE
        assert len(sk.download_packed([], recipient=True)) == 0                       # n = 0 -> 0
        assert L.fhs_download_string_packed_for(sk.ctx._h, None, 0, None, None, None, None) == 0
        p, one = PackedFheString.empty(3), np.zeros((1, N), U64)
        h = sk.ctx._h
        args = (h, _harr(s.chars), 3, p.mask16.ctypes.data, p.body16.ctypes.data)
        assert L.fhs_download_string_packed_for(*args, one.ctypes.data, None) == -1   # both 64-bit outputs or neither
        assert L.fhs_download_string_packed_for(h, None, 3, p.mask16.ctypes.data, p.body16.ctypes.data, None, None) == -1
        assert L.fhs_download_string_packed_for(None, None, 0, None, None, None, None) == -1
        assert L.fhs_debug_rekey_packed_device(h, None, None, 0, None, None) == FHS_ERR_STATE
        assert L.fhs_debug_rekey_packed_device(h, None, None, 4, None, None) == -1
    finally:
        sk.close()
    key = np.zeros(REKEY_KEY_WORDS, U64)
    assert L.fhs_rekey_packed_host(None, None, None, 0, None, None) == -1
    assert L.fhs_rekey_packed_host(key.ctypes.data, None, None, 0, None, None) == 0
    assert L.fhs_rekey_packed_host(key.ctypes.data, None, None, 4, None, None) == -1


def test_bindings_are_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(ROOT, "bindings", "fhestring_hip.rs")).read()
    for name in ("fhs_download_string_packed_for", "fhs_rekey_packed_host", "fhs_debug_rekey_packed_device"):
        assert name in text, name
