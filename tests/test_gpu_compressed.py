"""Compressed (seeded) ciphertexts and server keys on the MI355X: the device ChaCha20 against the host generator, the
device expansion of seeded strings against the host reference in every word, string ops on compressed uploads against
the same ops on classic uploads bit for bit, and the compressed server key expanded on the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RFC_KEY = [int.from_bytes(bytes(range(4 * i, 4 * i + 4)), "little") for i in range(8)]
RFC_NONCE = [0x09000000, 0x4A000000, 0x00000000]
RFC_BLOCK_1 = [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
               0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]


@pytest.fixture(scope="module")
def ck():
    from fhestring_amd.api import MyClientKey
    k = MyClientKey(0xC5EED)
    yield k
    k.close()


@pytest.fixture(scope="module")
def sk(ck):
    from fhestring_amd.api import MyServerKey
    s = MyServerKey.from_client_key(ck, arith=1)
    s.set_mode(1)
    yield s
    s.close()


def _host_stream(key, counter, nonce, n):
    import fhestring_amd
    L = fhestring_amd.lib()
    k, nn = np.array(key, np.uint32), np.array(nonce, np.uint32)
    out = np.zeros(n, np.uint64)
    L.fhs_chacha20_stream(k.ctypes.data, counter, nn.ctypes.data, out.ctypes.data, n)
    return out


def test_device_keystream_equals_the_host_generator(sk):
    dev = sk.ctx.chacha20_device(RFC_KEY, 1, RFC_NONCE, 4000)
    assert [int(w) for d in dev[:8] for w in (d & 0xFFFFFFFF, d >> 32)] == RFC_BLOCK_1      # RFC 8439 section 2.3.2
    assert np.array_equal(dev, _host_stream(RFC_KEY, 1, RFC_NONCE, 4000))
    # across the 32-bit counter's wrap: the carry goes into nonce[0] above the domain byte, as in Rng::refill
    start = 0xFFFFFFF3
    dev = sk.ctx.chacha20_device(RFC_KEY, start, [4, 77, 1], 1001)
    assert np.array_equal(dev, _host_stream(RFC_KEY, start, [4, 77, 1], 1001))


def test_device_expansion_equals_host_expansion(ck, sk):
    """Every word of every block at 1, 5, 300 and 4097 characters in one item (the GPU suite's item count is capped in
    conftest.py); 4097 characters = 16 388 blocks take several staging passes."""
    for n in (1, 5, 300, 4097):
        rng = np.random.default_rng(n)
        text = "".join(chr(c) for c in rng.integers(1, 128, max(1, n - 1)))[:n - 1] if n > 1 else ""
        c = ck.encrypt_compressed(text, n - len(text))
        assert len(c) == n, ("characters", n)
        got = sk.upload_compressed_string(c).download()
        want = c.expand()
        assert np.array_equal(got, want), ("characters", n)
        if n == 300:                                  # a rank's window of a sharded string
            assert np.array_equal(sk.upload_compressed_string(c, 100, 150).download(), want[100:250]), ("window of", n)
        assert ck.decrypt_str_raw(got) == text, ("characters", n)


def test_ops_on_compressed_uploads_match_classic_uploads_bit_for_bit(ck, sk):
    text, other = "The quick Brown fox jumps", "the QUICK brown FOX JUMPS"
    a, b = ck.encrypt_compressed(text, 1), ck.encrypt_compressed(other, 1)
    comp = (sk.upload_compressed_string(a), sk.upload_compressed_string(b))
    clas = (sk.upload_string(a.expand()), sk.upload_string(b.expand()))
    pat = ck.encrypt_str_raw("fox", 0)
    results = []
    for s, t in (comp, clas):
        p = sk.upload_string(pat).chars          # an encrypted pattern uploaded the classic way: a mixed flush
        r = [sk.contains_clear(s, "Brown"), sk.find(s, p), sk.eq_ignore_case(s, t)]
        up = sk.to_upper(s)
        results.append(([x.download() for x in r], up.download(), r, up))
    (rc, uc, r, up), (rk, uk, _, _) = results
    assert all(np.array_equal(x, y) for x, y in zip(rc, rk)) and np.array_equal(uc, uk)
    assert [ck.decrypt_char(x) for x in r] == [1, text.find("fox"), 1]
    assert ck.decrypt(up) == text.upper()


@pytest.mark.parametrize("arith", [0, 1])
def test_compressed_server_key_on_the_device(ck, tmp_path, arith):
    """Kind 4 file expanded on the device == the host expansion loaded as raw keys, bit for bit in both arithmetics."""
    import fhestring_amd
    from fhestring_amd.api import MyServerKey, expand_compressed_server_key
    from oracle import radix
    path = tmp_path / "compressed.key"
    ck.save_compressed_server_key(path)
    bsk, ksk = expand_compressed_server_key(*ck.compressed_server_key())
    dev = MyServerKey.from_compressed_key_file(path, arith=arith)
    host = MyServerKey.from_raw_keys(bsk, ksk, arith=arith)
    try:
        names = ["msg", "eq_biv", "sign"]
        luts = np.stack([radix.lut_poly(n) for n in names])
        cts = np.stack([ck.encrypt_char_raw(v)[k] for v in (0x00, 0x5A, 0xC3, 0xFF) for k in range(4)])
        idx = np.arange(cts.shape[0], dtype=np.uint32) % 3
        assert np.array_equal(dev.ctx.pbs_batch(cts, idx, luts), host.ctx.pbs_batch(cts, idx, luts))
        assert np.array_equal(dev.ctx.keyswitch_modswitch_batch(cts), host.ctx.keyswitch_modswitch_batch(cts))
        out = dev.ctx.pbs_batch(cts, np.zeros(cts.shape[0], np.uint32), luts[:1])
        assert [ck.decrypt_char_raw(out[4 * i:4 * i + 4]) for i in range(4)] == [0x00, 0x5A, 0xC3, 0xFF]
        if arith == 1:
            dev.set_mode(1)
            s = dev.upload_compressed_string(ck.encrypt_compressed("compressed keys", 1))
            assert ck.decrypt_char(dev.contains_clear(s, "keys")) == 1
        else:
            with pytest.raises(fhestring_amd.FhsError):
                MyServerKey.from_key_file(path)          # fhs_load_server_key_file refuses kind 4
    finally:
        dev.close()
        host.close()
