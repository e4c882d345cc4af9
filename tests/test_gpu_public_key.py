"""Public-key (compact) strings on the MI355X: the device's sample extraction against the host reference in every word
(whole strings and windows, across group boundaries and staging passes), string ops on public-key uploads against the
same ops on classic uploads of the host expansion bit for bit, a flush that mixes all three upload paths, the noise
bookkeeping, a packed download of a result, and the CLI.  Loops instead of parametrisation (the GPU suite's item count
is capped in conftest.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from fhestring_amd.api import MyClientKey
    k = MyClientKey(0xC5EED)
    yield k
    k.close()


@pytest.fixture(scope="module")
def pp(ck):
    from fhestring_amd.api import PublicParameters
    p = PublicParameters.from_bytes(ck.get_public_parameters().to_bytes())    # no secret on the encrypting side
    p.set_insecure_seed(12)
    yield p
    p.close()


def _server(ck, arith):
    from fhestring_amd.api import MyServerKey
    s = MyServerKey.from_client_key(ck, arith=arith)
    s.set_mode(1)
    return s


@pytest.fixture(scope="module")
def sk(ck):
    s = _server(ck, 1)
    yield s
    s.close()


def _ascii(rng, n):
    return "".join(chr(c) for c in rng.integers(1, 128, n))


def test_device_expansion_equals_host_expansion(ck, pp, sk):
    """Every word of every block.  513 characters end in a second group of four blocks; 4097 characters = 16 388 blocks
    take five staging passes that start inside a group; the windows start and end inside groups."""
    for n, windows in ((1, ()), (5, ()), (300, ((100, 150),)), (513, ()), (4097, ((500, 30),))):
        text = _ascii(np.random.default_rng(n), n - 1)
        c = pp.encrypt(text, 1)
        assert len(c) == n
        want = c.expand()
        got = sk.upload_compact_string(c).download()
        assert np.array_equal(got, want), n
        for first, count in windows:
            assert np.array_equal(sk.upload_compact_string(c, first, count).download(), want[first:first + count]), (n, first)
        assert ck.decrypt_str_raw(got) == text
    assert len(sk.upload_compact_string(c, 4097, 0)) == 0


def test_ops_on_public_key_uploads_match_classic_uploads_bit_for_bit(ck, pp):
    text, other = "The quick Brown fox jumps", "the QUICK brown FOX JUMPS"
    a, b = pp.encrypt(text, 1), pp.encrypt(other, 1)
    pat = pp.encrypt("fox", 0)
    for arith in (1, 0):
        sk = _server(ck, arith)
        try:
            pub = (sk.upload_compact_string(a), sk.upload_compact_string(b), sk.upload_compact_string(pat).chars)
            clas = (sk.upload_string(a.expand()), sk.upload_string(b.expand()), sk.upload_string(pat.expand()).chars)
            results = []
            for s, t, p in (pub, clas):
                r = [sk.contains_clear(s, "Brown"), sk.find(s, p), sk.eq_ignore_case(s, t)]
                up = sk.to_upper(s)
                results.append(([x.download() for x in r], up.download(), r, up))
            (rp, upp, r, up), (rk, uk, _, _) = results
            assert all(np.array_equal(x, y) for x, y in zip(rp, rk)) and np.array_equal(upp, uk), arith
            assert [ck.decrypt_char(x) for x in r] == [1, text.find("fox"), 1], arith
            assert ck.decrypt(up) == text.upper()
        finally:
            sk.close()


def test_mixed_flush_of_all_three_upload_paths(ck, pp, sk):
    text, other = "public, seeded and classic", "PUBLIC, SEEDED AND CLASSIC"
    s = sk.upload_compact_string(pp.encrypt(text, 1))                        # public-key string
    t = sk.upload_compressed_string(ck.encrypt_compressed(other, 1))        # seeded-compressed second string
    p = sk.upload_string(ck.encrypt_str_raw("seeded", 0)).chars             # classic pattern
    r = [sk.eq_ignore_case(s, t), sk.find(s, p), sk.contains(t, p), sk.eq(s, t)]
    sk.flush()
    assert [ck.decrypt_char(x) for x in r] == [1, text.find("seeded"), 0, 0]


def test_noise_bookkeeping_and_packed_download(ck, pp, sk):
    text = "packed results of a public-key upload"
    s = sk.upload_compact_string(pp.encrypt(text, 2))
    assert [ch.sum_c2() for ch in s.chars] == [1] * len(s)                   # fhs_char_sum_c2: one fresh encryption
    sk.load_packing_key(ck)
    up = sk.to_upper(s)
    assert ck.decrypt_packed(sk.download_packed(up)) == text.upper()
    assert ck.decrypt(up) == text.upper()


def test_cli_with_public_key_all_methods_pass(capsys):
    """The README's invocation with --public-key: every input string goes through PublicParameters."""
    from fhestring_amd import cli
    rc = cli.main(["--string", "hello", "--pattern", "ello", "--n", "1", "--from", "ello", "--to", "_llo", "--public-key"])
    text = capsys.readouterr().out
    assert rc == 0, text
    assert "Test Failed" not in text
    assert text.count("Test Passed: OK") >= len(cli.METHODS)
    assert 'Test Passed: OK, Result: "h_llo", Replace ' in text
    assert "Test Passed: OK, Result: 1, Find " in text
