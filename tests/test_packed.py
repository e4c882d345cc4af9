"""Packed result download on the host: the client's packing key and packed decryption, the public-data-only host
reference of the ring packing (fhs_pack_host / fhs_pack_switch16), one tree node against a schoolbook restatement of
the formulas in wrapping uint64, the noise the packing adds, sizes, formats and states."""
import math
import os
import random

import numpy as np
import pytest

from pack_model import node_dense as _node_schoolbook      # the schoolbook node, the key rounded to its grid first
from ring_util import glwe_phases

N = 2048
GLWE_NOISE = 2.9403601535432533e-16          # client.cpp: GLWE noise as a fraction of the torus (packing key, fresh blocks)
PACK_BASE_LOG, PACK_LEVELS = 16, 3
CLASSIC_4097_BYTES = 268632096               # 4097 characters x 4 blocks x 2049 words x 8 B
FHS_ERR_STATE = -3


@pytest.fixture(scope="module")
def ck():
    from fhestring_amd.api import MyClientKey
    k = MyClientKey(4242)
    yield k
    k.close()


def _ascii(rng, n):
    return "".join(chr(rng.randrange(1, 128)) for _ in range(n))


def _predicted_pack_sigma():
    """V_ks (N^2 - 1) / 3 plus the pre-scaling's N^2 (1 + N / 2) / 12"""
    s2 = (GLWE_NOISE * 2.0 ** 64) ** 2
    v_ks = PACK_LEVELS * N * (2.0 ** (2 * PACK_BASE_LOG) / 12) * s2 + (N / 2) * 2.0 ** (2 * (64 - PACK_LEVELS * PACK_BASE_LOG)) / 12
    return math.sqrt(v_ks * (N * N - 1) / 3 + N * N * (1 + N / 2) / 12)


def test_round_trip(ck):
    """1, 512 and 513 characters (4, 2048 and 2052 blocks) with paddings 0 / 1 / 7: pack_host -> switch16 -> decrypt_packed
    equals the classic decryption; block values with carries (0..15) and trivial blocks come back block by block."""
    from fhestring_amd.api import pack_host, pack_switch16
    rng = random.Random(5)
    key = ck.packing_key()
    for total in (1, 512, 513):
        for padding in (0, 1, 7):
            if padding > total:
                continue
            text = _ascii(rng, total - padding)
            ct = ck.encrypt_str_raw(text, padding)
            m64, b64 = pack_host(key, ct)
            p = pack_switch16(m64, b64, 4 * total)
            assert len(p) == total and p.mask16.shape == ((4 * total + 2047) // 2048, N)
            assert ck.decrypt_packed(p) == ck.decrypt_str_raw(ct) == text
            want = np.array([(ord(ch) >> (2 * b)) & 3 for ch in text + "\0" * padding for b in range(4)], np.uint8)
            assert np.array_equal(ck.decrypt_packed_blocks(p), want)
    # a single character with padding 0 at total 1 is covered above; blocks that carry: every value 0..15, twice, and
    # trivial blocks (0, v 2^59) between them
    vals = np.array(list(range(16)) * 2 + [3, 9, 15, 0], np.uint8)
    blocks = ck.encrypt_blocks_raw(vals)
    blocks[32:, :] = 0
    blocks[32:, N] = vals[32:].astype(np.uint64) << np.uint64(59)
    m64, b64 = pack_host(key, blocks)
    p = pack_switch16(m64, b64, len(vals))
    assert np.array_equal(ck.decrypt_packed_blocks(p), vals)


def test_one_node_against_schoolbook(ck):
    """One AutoKS + merge of two random GLWEs from the formulas in numpy's wrapping uint64 equals the library's node bit
    for bit, at the first, a middle and the last tree level; so does a 2-block pack (21 live nodes) restated node by
    node."""
    import ctypes as C
    import fhestring_amd
    from fhestring_amd.api import pack_host
    L = fhestring_amd.lib()
    key = np.array(ck.packing_key())
    rng = np.random.default_rng(77)
    for lv in (1, 6, 11):
        e = rng.integers(0, 1 << 64, (2, N), dtype=np.uint64)
        o = rng.integers(0, 1 << 64, (2, N), dtype=np.uint64)
        got = np.zeros((2, N), np.uint64)
        assert L.fhs_debug_pack_node(key.ctypes.data, lv, e.ctypes.data, o.ctypes.data, got.ctypes.data) == 0
        assert np.array_equal(got, _node_schoolbook(key, lv, e, o)), lv
    assert L.fhs_debug_pack_node(key.ctypes.data, 12, e.ctypes.data, o.ctypes.data, got.ctypes.data) == -1
    # two blocks: block 0 walks down the even side, block 1 sits at node 1 of every level until they meet at level 11
    blocks = ck.encrypt_blocks_raw([2, 13])

    def leaf(b):
        pre = (b + np.uint64(1 << 10)) >> np.uint64(11)
        g = np.zeros((2, N), np.uint64)
        g[0, 0] = pre[0]
        g[0, 1:] = (np.uint64(0) - pre[1:N])[::-1]          # A_{N-i} = -a_i
        g[1, 0] = pre[N]
        return g
    zero = np.zeros((2, N), np.uint64)
    n0, n1 = leaf(blocks[0]), leaf(blocks[1])
    for lv in range(1, 11):
        n0, n1 = _node_schoolbook(key, lv, n0, zero), _node_schoolbook(key, lv, n1, zero)
    top = _node_schoolbook(key, 11, n0, n1)
    m64, b64 = pack_host(key, blocks)
    assert np.array_equal(m64[0], top[0]) and np.array_equal(b64[0], top[1])


def test_noise_of_a_full_group(ck):
    """2048 fresh blocks: before the storage switch the error of coefficient j against m_j 2^59 stays under 2^46 and
    within a factor 2 of the derived figure; after it, the rounding to 16 bits dominates as derived."""
    from fhestring_amd.api import pack_host, pack_switch16
    rng = np.random.default_rng(3)
    vals = rng.integers(0, 16, 2048).astype(np.uint8)
    blocks = ck.encrypt_blocks_raw(vals)
    m64, b64 = pack_host(ck.packing_key(), blocks)
    _, glwe_sk = ck.secret_keys()
    want = vals.astype(np.uint64) << np.uint64(59)
    err = (glwe_phases(m64[0], b64[0], glwe_sk) - want).view(np.int64).astype(np.float64)
    sigma, predicted = float(err.std()), _predicted_pack_sigma()
    print("packing sigma: measured 2^%.2f, derived 2^%.2f" % (math.log2(sigma), math.log2(predicted)))
    assert abs(math.log2(predicted) - 43.1) < 0.1                # the figure DESIGN.md section 11 quotes
    assert sigma < 2.0 ** 46
    assert predicted / 2 < sigma < predicted * 2
    p = pack_switch16(m64, b64, 2048)
    m16 = p.mask16.astype(np.uint64) << np.uint64(48)
    b16 = np.zeros(N, np.uint64)
    b16[:2048] = p.body16.astype(np.uint64) << np.uint64(48)
    err16 = (glwe_phases(m16[0], b16, glwe_sk) - want).view(np.int64).astype(np.float64)
    unit = 2.0 ** 48 * math.sqrt((1 + float(glwe_sk.sum())) / 12)
    print("after the 16-bit switch: sigma 2^%.2f, derived 2^%.2f, max 2^%.2f" %
          (math.log2(err16.std()), math.log2(unit), math.log2(np.abs(err16).max())))
    assert 0.8 * unit <= err16.std() <= 1.2 * unit
    assert np.abs(err16).max() < 2.0 ** 56


def test_sizes_and_formats(ck, tmp_path):
    import ctypes as C
    import fhestring_amd
    from fhestring_amd.api import FhsError, MyClientKey, MyServerKey, PackedFheString, PACK_KEY_WORDS
    L = fhestring_amd.lib()
    p = PackedFheString.empty(4097)
    header = 16
    assert p.nbytes == header + 69640 == len(p.to_bytes())
    assert CLASSIC_4097_BYTES / p.nbytes > 3800
    mw, bw = C.c_size_t(), C.c_size_t()
    L.fhs_packed_bytes(4097, C.byref(mw), C.byref(bw))
    assert 2 * (mw.value + bw.value) == 69640 == 4096 * 9 + 2 * 4 * 4097
    q = PackedFheString(3, np.arange(N, dtype=np.uint16), np.arange(12, dtype=np.uint16))
    r = PackedFheString.from_bytes(q.to_bytes())
    assert len(r) == 3 and np.array_equal(r.mask16, q.mask16) and np.array_equal(r.body16, q.body16)
    data = q.to_bytes()
    for bad in (data[:-1], data + b"\0", data[:20], b"FHSCSTR1" + data[8:], b""):
        with pytest.raises(ValueError):
            PackedFheString.from_bytes(bad)
    with pytest.raises(ValueError):
        PackedFheString(513, np.zeros((1, N), np.uint16), np.zeros(2052, np.uint16))   # 2052 blocks need two groups

    bsk, ksk = np.array(ck.bsk()[:4096]), np.array(ck.ksk()[:4096])
    fresh = MyClientKey(4242)                                    # the packing key is generated on first use ...
    try:
        b0, k0 = np.array(fresh.bsk()), np.array(fresh.ksk())
        key = np.array(fresh.packing_key())
        assert np.array_equal(fresh.bsk(), b0) and np.array_equal(fresh.ksk(), k0)   # ... and moves nothing
        assert np.array_equal(b0[:4096], bsk) and np.array_equal(k0[:4096], ksk)
        assert key.size == PACK_KEY_WORDS == 11 * 3 * 2 * 2048 and np.array_equal(key, ck.packing_key())
        assert not (key & np.uint64(63)).any()                   # on the bootstrapping key's 58-bit grid
    finally:
        fresh.close()
    path = tmp_path / "pack.key"
    ck.save_packing_key(path)
    assert os.path.getsize(path) == 64 + PACK_KEY_WORDS * 8 == 1081408
    raw = np.fromfile(path, np.uint64)
    assert raw[1] == 5 and np.array_equal(raw[8:], ck.packing_key())
    with pytest.raises(FhsError):
        MyClientKey.load(path)
    planner = MyServerKey.planner()
    try:
        assert L.fhs_load_server_key_file(planner.ctx._h, str(path).encode()) == FHS_ERR_STATE
        assert L.fhs_load_multibit_key_file(planner.ctx._h, str(path).encode()) == FHS_ERR_STATE
        assert L.fhs_load_compressed_server_key_file(planner.ctx._h, str(path).encode()) == FHS_ERR_STATE
        other = tmp_path / "server.key"
        ck.save(other, server_key_only=True)
        assert L.fhs_load_packing_key_file(planner.ctx._h, str(other).encode()) == FHS_ERR_STATE
        assert L.fhs_load_packing_key_file(planner.ctx._h, str(path).encode()) == 0   # a planner holds no key: accepted, unused
    finally:
        planner.close()


def test_planner_context_refuses_a_packed_download(ck):
    from fhestring_amd.api import FhsError, MyServerKey
    sk = MyServerKey.planner()
    try:
        sk.load_packing_key(ck)
        s = sk.dummy_string(3)
        with pytest.raises(FhsError) as e:
            sk.download_packed(s)
        assert e.value.code == FHS_ERR_STATE
    finally:
        sk.close()
