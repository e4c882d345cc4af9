"""Packed result download on the MI355X: the device's ring packing against the host reference in every word (64-bit
GLWEs and 16-bit output; trivial, linear-combination and materialised handles in one string), string ops end to end
through the packed download in both modes and both bootstrap arithmetics, independence of the packed bytes from the
bootstrap arithmetic, and the state errors.  One client and one packing key for the module; every test its own
context(s); loops instead of parametrisation (the GPU suite's item count is capped in conftest.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2048
FHS_ERR_STATE = -3


@pytest.fixture(scope="module")
def ck():
    from fhestring_amd.api import MyClientKey
    k = MyClientKey(4242)
    k.packing_key()
    yield k
    k.close()


def _server(ck, arith, mode=1, packing_key=True):
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.from_client_key(ck, arith=arith)
    sk.set_mode(mode)
    if packing_key:
        sk.load_packing_key(ck)
    return sk


def _kinds(sk, ch):
    """kind of each of the four blocks of a handle: 0 plaintext, 1 block, 2 linear combination (fhs_debug_char_terms)"""
    n = C.c_size_t()
    buf = np.zeros(4096, np.uint64)
    sk.ctx._check(sk.ctx._L.fhs_debug_char_terms(sk.ctx._h, ch.h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)))
    kinds, i = [], 0
    while i < n.value:
        kinds.append(int(buf[i]))
        i += 3 + 2 * int(buf[i + 2])
    return kinds


def _ascii(rng, n):
    return "".join(chr(c) for c in rng.integers(1, 128, n))


def test_device_packing_equals_the_host_reference_in_every_word(ck):
    """1, 6, 300, 512 and 513 characters (6 and 300: 24 and 1200 blocks, a tree level at which some nodes have a live odd
    child and others do not -- level 7 with 16 nodes, 8 of them, and the leaf level with 1024, 176 of them; 6 rather
    than 3 or 5 characters because the loop body reads chars[4] and needs chars[3] != chars[n - 2]).  The longer strings
    hold a folded constant (TRIV), the result of if_then_else in fused mode (LIN: an unmaterialised sum of two bootstrap outputs per block; the packed download materialises it, as the
    classic one would) and uploaded blocks (MAT)."""
    from fhestring_amd.api import FheString, pack_host, pack_switch16
    rng = np.random.default_rng(6)
    key = ck.packing_key()
    sk = _server(ck, 0)
    try:
        for n in (1, 512, 513, 6, 300):                 # the new sizes last: the texts of the first three stay
            text = _ascii(rng, n)
            s = sk.upload_string(ck.encrypt_str_raw(text, 0))
            chars = list(s.chars)
            if n > 1:
                chars[3] = sk.trivial(ord("p")).add(sk.trivial(1))               # constant folding: stays plaintext
                chars[n - 2] = chars[0].eq(chars[1]).if_then_else(chars[2], chars[4])   # fused mode: a pending sum per block
                assert _kinds(sk, chars[3]) == [0] * 4 and _kinds(sk, chars[n - 2]) == [2] * 4
            s = FheString(chars)
            p, m64, b64 = sk.download_packed(s, wide=True)
            classic = s.download()                                                # after the packed one: same handles
            hm, hb = pack_host(key, classic)
            assert np.array_equal(m64, hm), n
            g = (4 * n + N - 1) // N
            for k in range(g):                                                    # body words of present blocks
                cnt = min(N, 4 * n - k * N)
                assert np.array_equal(b64[k, :cnt], hb[k, :cnt]), (n, k)
            assert np.array_equal(b64, hb), n                                     # ... and the rest of the polynomial
            hp = pack_switch16(hm, hb, 4 * n)
            assert np.array_equal(p.mask16, hp.mask16) and np.array_equal(p.body16, hp.body16), n
            assert p.to_bytes() == sk.download_packed(s).to_bytes()               # the plain entry point, same bytes
            raw = text.encode()
            want = [(v >> (2 * b)) & 3 for v in raw for b in range(4)]
            if n > 1:
                want[12:16] = [(ord("q") >> (2 * b)) & 3 for b in range(4)]
                picked = raw[2] if raw[0] == raw[1] else raw[4]
                want[4 * (n - 2):4 * (n - 1)] = [(picked >> (2 * b)) & 3 for b in range(4)]
            assert list(ck.decrypt_packed_blocks(p)) == want, n
    finally:
        sk.close()


def test_string_ops_through_the_packed_download(ck):
    """to_upper, replace (5 -> 5), trim, concatenate and find's index in both modes and both bootstrap arithmetics:
    packed and classic download decrypt to the Python result, and the classic download of the same handles is bit-equal
    before and after the packed one.  The index of find on a 208-character string is the noisiest handle the library
    hands back: its digits are unrefreshed sums (fhs_char_sum_c2 = 45 here; 57 is the bound documented in the header)."""
    from fhestring_amd.api import FheString
    rng = np.random.default_rng(7)
    long_text = "".join(chr(c) for c in rng.integers(97, 123, 204)) + "WXYZ"       # the pattern sits at the very end
    for arith in (0, 1):
        sk = _server(ck, arith)
        try:
            for mode in (0, 1):
                sk.set_mode(mode)
                enc = lambda t, pad=1: ck.encrypt(t, pad, None, sk)
                pat = lambda t: ck.encrypt_no_padding(t, sk)
                cases = [
                    (sk.to_upper(enc("Hi, yo")), "HI, YO"),
                    (sk.replace(enc("abcdeX"), pat("abcde"), pat("vwxyz")), "vwxyzX"),
                    (sk.trim(enc(" ab ")), "ab"),
                    (sk.concatenate(enc("ab"), enc("cd", 0)), "abcd"),
                ]
                for r, want in cases:
                    before = r.download()
                    p = sk.download_packed(r)
                    after = r.download()
                    assert np.array_equal(before, after), (arith, mode, want)
                    assert ck.decrypt_packed(p) == ck.decrypt_str_raw(before) == want, (arith, mode, want)
                finds = [(sk.find(enc("xxabxxab"), pat("ab")), 2)]
                if mode == 1:
                    idx = sk.find(enc(long_text), pat("WXYZ"))
                    assert idx.sum_c2() > 4                                       # unrefreshed digits: the noisy case
                    finds.append((idx, 204))
                for idx, want in finds:
                    r = FheString([idx])
                    before = r.download()
                    p = sk.download_packed(r)
                    assert np.array_equal(before, r.download()), (arith, mode, want)
                    blk = ck.decrypt_packed_blocks(p)
                    got = sum((int(blk[b]) & 15) << (2 * b) for b in range(4)) & 255
                    assert got == ck.decrypt_char_raw(before) == want, (arith, mode, want)
        finally:
            sk.close()


def test_packed_bytes_do_not_depend_on_the_bootstrap_arithmetic(ck):
    rng = np.random.default_rng(8)
    ct = ck.encrypt_str_raw(_ascii(rng, 40), 3)
    sk = _server(ck, 0)
    try:
        s = sk.upload_string(ct)
        exact = sk.download_packed(s).to_bytes()
        sk.ctx.set_arithmetic(1)
        assert sk.ctx.arithmetic == 1
        assert sk.download_packed(s).to_bytes() == exact
        assert sk.download_packed(sk.upload_string(ct)).to_bytes() == exact
    finally:
        sk.close()
    sk = _server(ck, 1)                                                           # a context that never was exact
    try:
        assert sk.download_packed(sk.upload_string(ct)).to_bytes() == exact
    finally:
        sk.close()


def test_states_and_key_file(ck, tmp_path):
    """No packing key: FHS_ERR_STATE.  The key comes as words or as a kind 5 file; a new server key drops it."""
    from fhestring_amd.api import FhsError
    sk = _server(ck, 1, packing_key=False)
    try:
        s = sk.upload_string(ck.encrypt_str_raw("state", 1))
        with pytest.raises(FhsError) as e:
            sk.download_packed(s)
        assert e.value.code == FHS_ERR_STATE
        path = tmp_path / "pack.key"
        ck.save_packing_key(path)
        sk.load_packing_key(path=path)
        assert ck.decrypt_packed(sk.download_packed(s)) == "state"
        assert len(sk.download_packed([])) == 0
        sk.ctx.load_server_key(ck.bsk(), ck.ksk())
        with pytest.raises(FhsError) as e:
            sk.download_packed(s)
        assert e.value.code == FHS_ERR_STATE
    finally:
        sk.close()


def test_a_second_server_key_takes_everything_derived_from_the_first_with_it(ck):
    """Reload on a context in the f64-FFT arithmetic that holds the pair key and the packing key of the first client: the
    Fourier-domain key is rebuilt from the NEW standard-domain key (two bootstraps, the smallest batch with a non-trivial
    pointer offset, decrypt under the second client's key), the pair key and the packing key are gone, close() is clean."""
    import noise_util as nu
    from fhestring_amd.api import FhsError, MyClientKey
    from oracle import radix
    ck2 = MyClientKey(4243)
    sk = _server(ck, 1)
    try:
        ctx = sk.ctx
        ctx.load_multibit_key(ck.bsk_mb2())
        ctx.set_arithmetic(ctx.ARITH_F64_FFT_MB2)                                 # the pair key is there ...
        ctx.set_arithmetic(ctx.ARITH_F64_FFT)
        s = sk.upload_string(ck.encrypt_str_raw("ab", 0))
        assert ck.decrypt_packed(sk.download_packed(s)) == "ab"                   # ... and so is the packing key
        ctx.load_server_key(ck2.bsk(), ck2.ksk())
        msgs = np.array([1, 2], np.uint64)
        cts = np.stack([ck2.encrypt_char_raw(int(m))[0] for m in msgs])           # block 0 of the char = m & 3
        got = ctx.pbs_batch(cts, np.zeros(2, np.uint32), radix.lut_poly("msg")[None, :])
        _, glwe_sk2 = ck2.secret_keys()
        e = nu.centred(nu.big_phase(got, glwe_sk2) - (msgs << np.uint64(59)), 64)
        assert np.abs(e).max() < 2 ** 53, np.abs(e)                               # 1/64 of a message step, as test_gpu_margins
        with pytest.raises(FhsError, match="pair key") as err:
            ctx.set_arithmetic(ctx.ARITH_F64_FFT_MB2)
        assert err.value.code == FHS_ERR_STATE and ctx.arithmetic == ctx.ARITH_F64_FFT
        with pytest.raises(FhsError) as err:
            sk.download_packed(s)
        assert err.value.code == FHS_ERR_STATE
    finally:
        sk.close()
        ck2.close()
    assert sk.ctx._h is None
