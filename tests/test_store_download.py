"""Packed download of parked store entries, own or recipient key, on the host (include/fhestring_hip.h, "string store:
packed download of parked entries"): fhs_store_packed_host against the existing references
fhs_pack_switch16 / fhs_rekey_packed_host applied to the entry's words << 32 and sliced to the window, every window shape
that reaches an edge, the flow from a public-key encryption to a's and b's decryption with the noise, the _at forms of the
client decryption, the ABI edges on a planner context, the binding and the serialised forms.  The device kernels are
compared with the host reference, word for word, in smoke() of __graft_entry__.py (tests/test_store_download_device.py
runs that step alone)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from ring_util import packed_phases

N = 2048
FHS_ERR_ARG, FHS_ERR_STATE = -1, -3
U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5A5
PAD = 64                                                             # sentinel words on either side of an output array
# 32-bit words on the rounding boundaries of the own-key switch -> the 16-bit word each must give
ROUNDING = ((0x00007FFF, 0x0000), (0x00008000, 0x0001), (0x7FFF8000, 0x8000), (0xFFFF7FFF, 0xFFFF), (0xFFFF8000, 0x0000))
# 32-bit mask words on the digit boundaries of the keyswitch (the re-key's: DESIGN.md section 14)
DIGITS = (0x00000000, 0x00008000, 0x7FFF8000, 0x80000000, 0xFFFFFFFF, 0x00007FFF)
ENTRIES = (513, 1026, 2561)                                          # 2 / 3 / 6 groups, the last holding 4 / 8 / 4 blocks


def windows(n):
    """(first_char, count) of every window shape that reaches an edge, as far as it lies inside n characters"""
    w = [(0, n), (0, 1), (511, 1), (511, 2), (512, 1), (512, 512), (n - 1, 1)]
    if n == 1026:
        w.append((511, 514))                                         # three covering groups, first and last partial
    return [x for x in w if x[0] + x[1] <= n]


def sizes(first_char, count):
    """the formulas of the windowed packed form: (mask words, body words, first_coef, g0)"""
    t0 = 4 * first_char
    g0, g1 = t0 // N, (t0 + 4 * count - 1) // N
    return (g1 - g0 + 1) * N, 4 * count, t0 % N, g0


def random_entry(rng, n_chars, chosen=None):
    from fhestring_amd.api import CompactFheString
    g = (4 * n_chars + N - 1) // N
    mask = rng.integers(0, 1 << 32, (g, N), dtype=np.uint32)
    body = rng.integers(0, 1 << 32, 4 * n_chars, dtype=np.uint32)
    if chosen is not None and g == len(chosen):                      # the six-group entry: one chosen word per group,
        mask[:] = np.array(chosen, np.uint32)[:, None]               # throughout its mask and at the group's first bodies
        for k, w in enumerate(chosen):
            body[k * N:k * N + 4] = w
    return CompactFheString(n_chars, mask, body)


def wide(c):
    """the entry's words << 32 as the [groups][2048] arrays the 64-bit references take"""
    body = np.zeros(c.mask32.shape, U64)
    body.reshape(-1)[:4 * len(c)] = c.body32.astype(U64) << U64(32)
    return c.mask32.astype(U64) << U64(32), body


def check_window(got, whole, first_char, count, what):
    mw, bw, fc, g0 = sizes(first_char, count)
    assert (got.first_coef, got.mask16.size, got.body16.size) == (fc, mw, bw), what
    assert np.array_equal(got.mask16, whole.mask16[g0:g0 + mw // N]), what
    assert np.array_equal(got.body16, whole.body16[4 * first_char:4 * (first_char + count)]), what


@pytest.fixture(scope="module")
def clients():
    from fhestring_amd.api import MyClientKey
    a, b = MyClientKey(0x5EEDA), MyClientKey(0x5EEDB)
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def flow(clients):
    """A 513-character string encrypted under a's PUBLIC key (no GPU, no secret): what fhs_store_import parks as it
    arrives; and one re-key key a -> b.  Computed once, left unchanged."""
    a, b = clients
    text = "".join(chr(33 + (7 * i) % 90) for i in range(513))
    pp = a.get_public_parameters()
    pp.set_insecure_seed(17)
    c = pp.encrypt(text, 0)
    c.mask32.setflags(write=False)
    c.body32.setflags(write=False)
    return a, b, text, c, a.rekey_key(b)


def test_sizes():
    from fhestring_amd.api import store_packed_words
    for n in ENTRIES:
        for first, count in windows(n) + [(3, 700), (1023, 2)]:
            assert store_packed_words(first, count) == sizes(first, count)[:3], (first, count)
            assert store_packed_words(first, count)[2] % 4 == 0
    assert store_packed_words(0, 513) == (2 * N, 2052, 0)            # first_char = 0: fhs_packed_bytes
    assert store_packed_words(5, 0)[:2] == (0, 0)


def test_own_key_equals_the_storage_switch_of_the_words_shifted_left():
    from fhestring_amd.api import pack_switch16, store_packed_host
    rng = np.random.default_rng(170)
    for n in ENTRIES:
        c = random_entry(rng, n, [w for w, _ in ROUNDING] + [0x12348000])   # six groups: one word each, and a tie upwards
        whole = pack_switch16(*wide(c), 4 * n)                       # the existing reference on words << 32
        one_liner = lambda w: (((w.astype(U64) + U64(1 << 15)) >> U64(16)) & U64(0xffff)).astype(np.uint16)
        assert np.array_equal(whole.mask16, one_liner(c.mask32)) and np.array_equal(whole.body16, one_liner(c.body32))
        for first, count in windows(n):
            check_window(store_packed_host(None, c, first, count), whole, first, count, (n, first, count))
    # the rounding boundaries, as masks and as bodies (the six-group entry carried one per group above; here by value)
    words = np.array([w for w, _ in ROUNDING], np.uint32)
    c = random_entry(rng, 513)
    c.mask32[0, :len(words)] = words
    c.body32[2044:2044 + len(words)] = words                         # across the boundary of groups 0 | 1
    got = store_packed_host(None, c, 511, 2)
    assert [int(x) for x in got.mask16[0, :len(words)]] == [want for _, want in ROUNDING]
    assert [int(x) for x in got.body16[:len(words)]] == [want for _, want in ROUNDING]


def test_recipient_equals_the_packed_rekey_of_the_words_shifted_left():
    from fhestring_amd.api import REKEY_KEY_WORDS, rekey_packed_host, store_packed_host
    rng = np.random.default_rng(171)
    key = rng.integers(0, 1 << 64, REKEY_KEY_WORDS, dtype=U64)
    for n in ENTRIES:
        c = random_entry(rng, n, DIGITS)
        whole = rekey_packed_host(key, *wide(c), 4 * n)              # switch32(m << 32) = m: the same keyswitch input
        for first, count in windows(n):
            check_window(store_packed_host(key, c, first, count), whole, first, count, (n, first, count))
    assert len(random_entry(rng, 2561, DIGITS).mask32) == len(DIGITS)
    # every digit-boundary word inside ONE mask too, at its first positions and then at random
    c = random_entry(rng, 513)
    c.mask32[0] = rng.choice(np.array(DIGITS, np.uint32), N)
    c.mask32[0, :len(DIGITS)] = DIGITS
    check_window(store_packed_host(key, c, 511, 2), rekey_packed_host(key, *wide(c), 4 * 513), 511, 2, "digit words")


def test_no_word_outside_the_window_is_written():
    import fhestring_amd
    from fhestring_amd.api import REKEY_KEY_WORDS, store_packed_host
    L = fhestring_amd.lib()
    rng = np.random.default_rng(172)
    key = rng.integers(0, 1 << 64, REKEY_KEY_WORDS, dtype=U64)
    for n in ENTRIES:
        c = random_entry(rng, n)
        for first, count in windows(n):
            mw, bw, _, _ = sizes(first, count)
            for k in (None, key):
                m16 = np.full(mw + 2 * PAD, SENTINEL, np.uint16)
                b16 = np.full(bw + 2 * PAD, SENTINEL, np.uint16)
                rc = L.fhs_store_packed_host(None if k is None else k.ctypes.data, c.mask32.ctypes.data, c.body32.ctypes.data,
                                             4 * n, first, count, m16[PAD:].ctypes.data, b16[PAD:].ctypes.data)
                assert rc == 0
                for arr, words in ((m16, mw), (b16, bw)):
                    assert (arr[:PAD] == SENTINEL).all() and (arr[PAD + words:] == SENTINEL).all(), (n, first, count)
                want = store_packed_host(k, c, first, count)
                assert np.array_equal(m16[PAD:PAD + mw], want.mask16.reshape(-1)) and np.array_equal(b16[PAD:PAD + bw], want.body16)
    c = random_entry(rng, 513)
    m16, b16 = np.full(2 * N, SENTINEL, np.uint16), np.full(2052, SENTINEL, np.uint16)
    args = (c.mask32.ctypes.data, c.body32.ctypes.data, 4 * 513)
    assert L.fhs_store_packed_host(None, *args, 512, 512, m16.ctypes.data, b16.ctypes.data) == FHS_ERR_ARG   # outside
    assert L.fhs_store_packed_host(None, *args, 514, 0, m16.ctypes.data, b16.ctypes.data) == FHS_ERR_ARG
    assert L.fhs_store_packed_host(None, *args, 513, 0, None, None) == 0                                     # nothing to do
    assert L.fhs_store_packed_host(None, *args, 0, 1, None, b16.ctypes.data) == FHS_ERR_ARG
    assert (m16 == SENTINEL).all() and (b16 == SENTINEL).all()


def test_the_flow_decrypts_under_the_own_key_and_under_the_recipients(flow):
    from fhestring_amd.api import store_packed_host
    a, b, text, c, key = flow
    for first, count in windows(513):
        own, rec = store_packed_host(None, c, first, count), store_packed_host(key, c, first, count)
        assert a.decrypt_packed(own) == text[first:first + count], (first, count)
        assert b.decrypt_packed(rec) == text[first:first + count], (first, count)
        want = np.array([(ord(ch) >> (2 * k)) & 3 for ch in text[first:first + count] for k in range(4)], np.uint8)
        assert np.array_equal(a.decrypt_packed_blocks(own), want) and np.array_equal(b.decrypt_packed_blocks(rec), want)
        try:
            wrong = a.decrypt_packed(rec)
        except UnicodeDecodeError:                                   # not even ASCII
            wrong = None
        assert wrong != text[first:first + count], (first, count)
        assert not np.array_equal(a.decrypt_packed_blocks(rec), want)


def test_noise(flow):
    """Phase error of the whole 513-character entry under the own key and under the recipient's.  Both are dominated by
    the 16-bit rounding, 2^48 sqrt((1 + |S|^2) / 12) ~ 2^51.2, under keys of equal weight (the entry's 2^35.2 and the
    keyswitch's 2^32.6 disappear under it), so each is within a factor 2 of the other -- section 16's criterion; decoding
    fails at 2^58 and 2^55, the bound of tests/test_recipient.py, is about 14 sigma of the derived figure."""
    from fhestring_amd.api import store_packed_host
    a, b, text, c, key = flow
    want = np.array([(ord(ch) >> (2 * k)) & 3 for ch in text for k in range(4)], U64) << U64(59)
    sa, sb = a.secret_keys()[1], b.secret_keys()[1]
    e_own = (packed_phases(store_packed_host(None, c), sa) - want).view(np.int64).astype(np.float64)
    e_rec = (packed_phases(store_packed_host(key, c), sb) - want).view(np.int64).astype(np.float64)
    s_own, s_rec = float(e_own.std()), float(e_rec.std())
    derived = 2.0 ** 48 * math.sqrt((1 + float(sb.sum())) / 12)
    print("store download: own-key sigma 2^%.2f, recipient sigma 2^%.2f, derived 2^%.2f, max |e| 2^%.2f / 2^%.2f" %
          (math.log2(s_own), math.log2(s_rec), math.log2(derived), math.log2(np.abs(e_own).max()), math.log2(np.abs(e_rec).max())))
    assert np.abs(e_own).max() < 2.0 ** 55 and np.abs(e_rec).max() < 2.0 ** 55
    assert s_own / 2 < s_rec < s_own * 2
    # a window's phases are the whole entry's, block for block: the window changes no word
    w = store_packed_host(key, c, 511, 2)
    assert np.array_equal(packed_phases(w, sb), packed_phases(store_packed_host(key, c), sb)[2044:2052])


def test_at_forms_of_the_client_decryption(clients):
    import fhestring_amd
    from fhestring_amd.api import pack_host, pack_switch16
    L = fhestring_amd.lib()
    a, _ = clients
    text = "window, first_coef = 0"
    n = len(text)
    p = pack_switch16(*pack_host(a.packing_key(), a.encrypt_str_raw(text, 0)), 4 * n)
    old, new = np.zeros(4 * n, np.uint8), np.full(4 * n, 99, np.uint8)
    m, b = p.mask16.ctypes.data, p.body16.ctypes.data
    assert L.fhs_client_decrypt_packed_blocks(a._h, m, b, 4 * n, old.ctypes.data) == 0
    assert L.fhs_client_decrypt_packed_blocks_at(a._h, m, b, 0, 4 * n, new.ctypes.data) == 0
    assert np.array_equal(old, new)
    bufs, lens = [C.create_string_buffer(n + 1) for _ in range(2)], [C.c_size_t() for _ in range(2)]
    assert L.fhs_client_decrypt_packed_str(a._h, m, b, n, bufs[0], C.byref(lens[0])) == 0
    assert L.fhs_client_decrypt_packed_str_at(a._h, m, b, 0, n, bufs[1], C.byref(lens[1])) == 0
    assert bufs[0].raw[:lens[0].value] == bufs[1].raw[:lens[1].value] == text.encode()
    for bad in (3, 2, 2048, 2052):                                   # a multiple of 4 below 2048, or FHS_ERR_ARG
        assert L.fhs_client_decrypt_packed_blocks_at(a._h, m, b, bad, 4 * n, new.ctypes.data) == FHS_ERR_ARG
        assert L.fhs_client_decrypt_packed_str_at(a._h, m, b, bad, n, bufs[1], C.byref(lens[1])) == FHS_ERR_ARG
    assert L.fhs_client_decrypt_packed_blocks_at(a._h, None, None, 4, 0, None) == 0


def test_planner_context_and_argument_errors():
    import fhestring_amd
    from fhestring_amd.api import FhsError, MyServerKey, REKEY_KEY_WORDS
    L = fhestring_amd.lib()
    sk = MyServerKey.planner()
    try:
        e = sk.store_put(sk.dummy_string(6))
        with pytest.raises(FhsError) as err:
            e.download_packed()
        assert err.value.code == FHS_ERR_STATE and "planner" in str(err.value)
        sk.load_rekey_key(np.zeros(REKEY_KEY_WORDS, U64))
        with pytest.raises(FhsError) as err:
            e.download_packed(2, 3, recipient=True)
        assert err.value.code == FHS_ERR_STATE
        assert len(e.download_packed(2, 0)) == 0                     # count = 0 -> 0
        assert L.fhs_store_download_packed(sk.ctx._h, e.id, 6, 0, 0, None, None) == 0
        m16, b16 = np.full(N, SENTINEL, np.uint16), np.full(24, SENTINEL, np.uint16)
        args = (m16.ctypes.data, b16.ctypes.data)
        assert L.fhs_store_download_packed(sk.ctx._h, e.id + 1, 0, 1, 0, *args) == FHS_ERR_ARG     # unknown id
        assert L.fhs_store_download_packed(sk.ctx._h, e.id, 5, 2, 0, *args) == FHS_ERR_ARG         # window outside the entry
        assert L.fhs_store_download_packed(sk.ctx._h, e.id, 7, 0, 0, *args) == FHS_ERR_ARG
        assert L.fhs_store_download_packed(sk.ctx._h, e.id, 0, 6, 0, None, b16.ctypes.data) == FHS_ERR_ARG
        assert L.fhs_store_download_packed(None, e.id, 0, 6, 0, *args) == FHS_ERR_ARG
        assert (m16 == SENTINEL).all() and (b16 == SENTINEL).all()
        assert e.rekeys == 0 and len(e) == 6
    finally:
        sk.close()


def test_bindings_are_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = open(os.path.join(ROOT, "bindings", "fhestring_hip.rs")).read()
    for name in ("fhs_store_download_packed", "fhs_store_packed_host", "fhs_store_packed_words",
                 "fhs_client_decrypt_packed_str_at", "fhs_client_decrypt_packed_blocks_at"):
        assert name in text, name


def test_serialised_forms(flow):
    from fhestring_amd.api import PackedFheString, store_packed_host
    a, b, text, c, key = flow
    p = store_packed_host(None, c)                                   # first_coef = 0: the format there was, byte for byte
    assert p.first_coef == 0
    old = b"FHSPSTR1" + np.uint64(513).tobytes() + p.mask16.tobytes() + p.body16.tobytes()
    assert p.to_bytes() == old and p.nbytes == len(old) == 16 + 2 * 4096 + 8 * 513
    q = PackedFheString.from_bytes(old)
    assert q.first_coef == 0 and a.decrypt_packed(q) == text
    w = store_packed_host(key, c, 511, 2)                            # a window: a magic of its own, the offset in the header
    data = w.to_bytes()
    assert data[:8] == b"FHSPSTW1" and len(data) == w.nbytes == 24 + 2 * 4096 + 16
    assert int(np.frombuffer(data, U64, 2, 8)[1]) == 2044
    r = PackedFheString.from_bytes(data)
    assert r.first_coef == 2044 and len(r) == 2 and r.to_bytes() == data
    assert b.decrypt_packed(r) == text[511:513]
    for bad in (data[:-2], b"FHSPSTW1" + np.array([2, 3], U64).tobytes() + data[24:],
                b"FHSPSTW1" + np.array([2, 0], U64).tobytes() + data[24:]):
        with pytest.raises(ValueError):
            PackedFheString.from_bytes(bad)
    with pytest.raises(ValueError):
        PackedFheString(2, w.mask16, w.body16, first_coef=2046)
