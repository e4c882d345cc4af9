"""Compressed (seeded) ciphertexts and server keys on the host: the client's seeded encryption, the public-data-only
expansion, the pinned stream convention of include/fhestring_hip.h, noise, seeds, sizes, validity of the compressed
server key under the CPU oracle, and the planner's view of a compressed upload."""
import random

import numpy as np
import pytest

GLWE_NOISE = 2.9403601535432533e-16          # client.cpp: the classic encryption's GLWE noise (fraction of the torus)
CLASSIC_CHAR_BYTES = 4 * 2049 * 8
KIND2_FILE_BYTES = 64 + (742 * 4 * 2048 + 2048 * 5 * 743) * 8
KIND4_FILE_BYTES = 24395872


@pytest.fixture(scope="module")
def ck():
    from fhestring_amd.api import MyClientKey
    k = MyClientKey(4242)
    yield k
    k.close()


def _ascii(rng, n):
    return "".join(chr(rng.randrange(1, 128)) for _ in range(n))


def _stream(seed, domain, sid, n, counter=0):
    import fhestring_amd
    L = fhestring_amd.lib()
    key = np.ascontiguousarray(seed, np.uint32)
    nonce = np.array([domain, sid & 0xFFFFFFFF, sid >> 32], np.uint32)
    out = np.zeros(n, np.uint64)
    L.fhs_chacha20_stream(key.ctypes.data, counter, nonce.ctypes.data, out.ctypes.data, n)
    return out


def test_round_trip_and_windows(ck):
    rng = random.Random(11)
    for padding in (0, 1, 7):
        text = _ascii(rng, rng.randrange(1, 90))
        c = ck.encrypt_compressed(text, padding)
        assert len(c) == len(text) + padding and c.bodies.shape == (len(c), 4)
        full = c.expand()
        assert full.shape == (len(c), 4, 2049)
        assert ck.decrypt_str_raw(full) == text
        assert np.array_equal(full[:, :, 2048], c.bodies)
        c0, c1 = len(c) // 3, len(c) - 1
        assert np.array_equal(c.expand(c0, c1 - c0), full[c0:c1])
    with pytest.raises(AssertionError):
        ck.encrypt_compressed("bad\0string", 1)


def test_pinned_stream_convention(ck):
    """Mask word k of (character i, block b) = draw k of the stream (seed, counter 0, nonce (4, lo, hi) of 4i + b); BSK
    rows: domain 5, stream 2i + r, masked to the 58-bit grid; KSK rows: domain 6, stream 5i + l, 742 draws."""
    from fhestring_amd.api import expand_compressed_server_key
    c = ck.encrypt_compressed("pinned", 1)
    full = c.expand()
    for i, b in ((0, 0), (3, 2), (6, 3)):
        assert np.array_equal(full[i, b, :2048], _stream(c.seed, 4, 4 * i + b, 2048))
    # the window of a sharded string draws from the GLOBAL character index
    assert np.array_equal(c.expand(5, 2)[0, 1, :2048], _stream(c.seed, 4, 4 * 5 + 1, 2048))
    seed, bb, kb = ck.compressed_server_key()
    bsk, ksk = expand_compressed_server_key(seed, bb, kb)
    bsk, ksk = bsk.reshape(742, 2, 2, 2048), ksk.reshape(2048, 5, 743)
    qmask = np.uint64(~63 & 0xFFFFFFFFFFFFFFFF)
    for i, r in ((0, 0), (0, 1), (741, 1)):
        assert np.array_equal(bsk[i, r, 0], _stream(seed, 5, 2 * i + r, 2048) & qmask)
        assert np.array_equal(bsk[i, r, 1], bb[i, r])
    for i, l in ((0, 0), (1000, 3), (2047, 4)):
        assert np.array_equal(ksk[i, l, :742], _stream(seed, 6, 5 * i + l, 742))
        assert ksk[i, l, 742] == kb[i, l]


def test_noise_matches_the_classic_encryption(ck):
    rng = random.Random(5)
    text = _ascii(rng, 1024)
    c = ck.encrypt_compressed(text, 0)
    full = c.expand().reshape(-1, 2049)
    assert full.shape[0] >= 4096
    _, glwe = ck.secret_keys()
    dot = full[:, :2048][:, glwe.astype(bool)].sum(axis=1, dtype=np.uint64)   # wraps mod 2^64
    msg = np.array([(ord(ch) >> (2 * b)) & 3 for ch in text for b in range(4)], np.uint64)
    err = (full[:, 2048] - dot - (msg << np.uint64(59))).view(np.int64).astype(np.float64)
    want = GLWE_NOISE * 2.0 ** 64
    assert 0.8 * want < err.std() < 1.2 * want, (err.std(), want)
    assert np.abs(err).max() < 2.0 ** 40          # decoding fails only beyond 2^58


def test_seeds_are_fresh_and_reproducible_only_for_insecure_clients():
    from fhestring_amd.api import MyClientKey
    a, b = MyClientKey(77), MyClientKey(77)
    s1, s2 = MyClientKey(), MyClientKey()
    try:
        x, y = a.encrypt_compressed("seed", 2), a.encrypt_compressed("seed", 2)
        assert not np.array_equal(x.seed, y.seed) and not np.array_equal(x.bodies, y.bodies)
        x2, y2 = b.encrypt_compressed("seed", 2), b.encrypt_compressed("seed", 2)
        assert np.array_equal(x.seed, x2.seed) and np.array_equal(x.bodies, x2.bodies)
        assert np.array_equal(y.seed, y2.seed) and np.array_equal(y.bodies, y2.bodies)
        assert np.array_equal(a.compressed_server_key()[0], b.compressed_server_key()[0])
        p, q = s1.encrypt_compressed("seed", 2), s2.encrypt_compressed("seed", 2)
        assert not np.array_equal(p.seed, q.seed) and not np.array_equal(p.bodies, q.bodies)
        assert not np.array_equal(s1.compressed_server_key()[0], s2.compressed_server_key()[0])
        assert s1.decrypt_str_raw(p.expand()) == "seed" and s2.decrypt_str_raw(q.expand()) == "seed"
    finally:
        for k in (a, b, s1, s2):
            k.close()


def test_sizes_serialisation_and_key_file(ck, tmp_path):
    import fhestring_amd
    from fhestring_amd.api import CompressedFheString, MyClientKey
    c = ck.encrypt_compressed("x" * 4096, 1)
    data = c.to_bytes()
    assert len(data) == 48 + 32 * len(c) == c.nbytes and data[:8] == b"FHSCSTR1"
    d = CompressedFheString.from_bytes(data)
    assert np.array_equal(d.seed, c.seed) and np.array_equal(d.bodies, c.bodies)
    with pytest.raises(ValueError):
        CompressedFheString.from_bytes(data[:-8])
    assert len(c) * CLASSIC_CHAR_BYTES / c.nbytes > 2040          # 4097 characters: 268 MB -> 131 KB
    path = tmp_path / "compressed.key"
    bsk, ksk = ck.bsk().copy(), ck.ksk().copy()
    ck.save_compressed_server_key(path)
    assert path.stat().st_size == KIND4_FILE_BYTES
    assert KIND2_FILE_BYTES / KIND4_FILE_BYTES > 4.4
    raw = path.read_bytes()
    seed, bb, kb = ck.compressed_server_key()
    assert raw[:8] == b"FHSKEY01" and np.frombuffer(raw, np.uint64, 1, 8)[0] == 4
    assert raw[64:96] == seed.tobytes() and raw[96:96 + bb.nbytes] == bb.tobytes() and raw[96 + bb.nbytes:] == kb.tobytes()
    assert np.array_equal(ck.bsk(), bsk) and np.array_equal(ck.ksk(), ksk)   # the classic key does not move
    with pytest.raises(fhestring_amd.FhsError):
        MyClientKey.load(path)


def test_compressed_server_key_bootstraps_correctly_under_the_oracle(ck):
    """A second valid server key of the same secret keys: the oracle PBS decrypts f(m) with its host expansion."""
    from fhestring_amd.api import expand_compressed_server_key
    from oracle import core, radix
    _, glwe = ck.secret_keys()
    bsk, ksk = expand_compressed_server_key(*ck.compressed_server_key())
    assert not np.array_equal(bsk, ck.bsk()) and not np.array_equal(ksk, ck.ksk())
    S = core.ServerKey(bsk, ksk)
    ch = ck.encrypt_char_raw(0b11100100)                   # blocks 0,1,2,3
    outs = S.pbs_batch(ch, np.zeros(4, np.uint32), radix.lut_poly("msg")[None])
    assert [int(core.lib().orc_decrypt_block(glwe, np.ascontiguousarray(o))) for o in outs] == [0, 1, 2, 3]


def test_planner_accepts_a_compressed_upload(ck):
    from fhestring_amd.api import MyServerKey
    c = ck.encrypt_compressed("planning a compressed upload", 1)
    got = []
    for compressed in (True, False):
        sk = MyServerKey.planner()
        sk.set_mode(1)
        s = sk.upload_compressed_string(c) if compressed else sk.upload_string(c.expand())
        assert len(s) == len(c)
        sk.stats(reset=True)
        r = sk.contains_clear(s, "compressed")
        sk.flush()
        st = sk.stats()
        got.append((st["pbs_executed"], st["levels"], sk.level_widths(), st["max_input_sum_c2"]))
        del r, s
        sk.close()
    assert got[0] == got[1] and got[0][0] > 0
