"""Device-resident string store on the MI355X: the parked words against the host reference (packing tree + 32-bit switch)
in every word, the restored blocks against the host expansion bit for bit (whole strings and windows), a put of more
than four groups (two tree batches: the switch kernel's group offset), string operations on restored strings in both
modes and both bootstrap arithmetics, the noise bookkeeping with real rotation groups, import of a public-key string,
states and lifetime.  One client and one packing key for the module; every test its own context(s); loops instead of
parametrisation (the GPU suite's item count is capped in conftest.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2048
FHS_ERR_ARG, FHS_ERR_STATE, FHS_ERR_LIMIT = -1, -3, -4


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


def _host_entry(key, classic):
    from fhestring_amd.api import pack_host, pack_switch32
    return pack_switch32(*pack_host(key, classic), 4 * classic.shape[0])


def _put_code(sk, chars):
    from fhestring_amd.api import FhsError
    try:
        sk.store_put(chars).drop()
    except FhsError as e:
        return e.code
    return 0


def test_device_entry_equals_the_host_reference_in_every_word(ck):
    """1, 6, 300, 512 and 513 characters (6 and 300: 24 and 1200 blocks -- a packing-tree level with mixed liveness of the
    odd children, and body quarters of 6 and 300 words, which end inside a workgroup of the switch).  The longer strings
    hold a folded constant (TRIV), the result of if_then_else in fused mode (LIN: put materialises it, as a download would) and uploaded blocks (MAT).  The exported entry is the host's
    packing + switch of the classic download; what get() restores is the host expansion of those words, whole and for
    the windows (510, 3) -- blocks 2040-2051, across the group boundary --, (1, 1) -- first coefficient 4, inside a
    workgroup's eight -- and (512, 1)."""
    from fhestring_amd.api import FheString
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
            e = sk.store_put(s)
            assert len(e) == n and e.device_bytes == 8192 * ((4 * n + N - 1) // N) + 16 * n
            classic = s.download()                                                # after the put: same handles
            host = _host_entry(key, classic)
            got, meta = e.export()
            assert np.array_equal(got.mask32, host.mask32), n
            assert np.array_equal(got.body32, host.body32), n
            want_meta = np.full(4 * n, 1 | 1 << 16, np.uint64)                    # figure 1, one packing, no group
            if n > 1:
                assert _kinds(sk, chars[3]) == [0] * 4 and _kinds(sk, chars[n - 2]) == [1] * 4
                want_meta[4 * (n - 2):4 * (n - 1)] = 2 | 1 << 16                  # the sum of two bootstrap outputs
            assert np.array_equal(meta, want_meta), n
            full = host.expand()
            assert np.array_equal(e.get().download(), full), n
            for first, count in ((510, 3), (1, 1), (512, 1), (0, 0)):
                if first + count <= n:
                    w = e.get(first, count)
                    assert len(w) == count
                    assert np.array_equal(w.download(), full[first:first + count]), (n, first, count)
            raw = bytearray(text.encode())
            if n > 1:
                raw[3] = ord("q")
                raw[n - 2] = raw[2] if raw[0] == raw[1] else raw[4]
            assert ck.decrypt_str_raw(e.get().download()) == raw.decode()
            if n > 1:
                back = e.get(n - 2, 1)[0]
                assert back.sum_c2() == chars[n - 2].sum_c2() == 2 and e.get(3, 1)[0].sum_c2() == 1
            e.drop()
    finally:
        sk.close()


def test_more_than_four_groups(ck):
    """2049 characters = 8196 blocks = five groups: two batches of the packing tree, the second writing group 4 of the
    entry, and three passes of the expansion."""
    rng = np.random.default_rng(9)
    key = ck.packing_key()
    sk = _server(ck, 1)
    try:
        text = "".join(chr(c) for c in rng.integers(32, 127, 2049))
        s = sk.upload_string(ck.encrypt_str_raw(text, 0))
        e = sk.store_put(s)
        assert e.device_bytes == 8192 * 5 + 16 * 2049
        host = _host_entry(key, s.download())
        got, meta = e.export()
        assert np.array_equal(got.mask32, host.mask32)
        assert np.array_equal(got.body32, host.body32)
        assert np.array_equal(meta, np.full(8196, 1 | 1 << 16, np.uint64))
        del s
        restored = e.get().download()
        assert np.array_equal(restored, host.expand())
        assert ck.decrypt_str_raw(restored) == text
        assert np.array_equal(e.get(2046, 3).download(), restored[2046:])         # the last group's four blocks and the group before
    finally:
        sk.close()


def test_operations_on_restored_strings(ck):
    """to_upper, contains_clear, eq against a twin that was never parked, and find on a restored string, in both modes and
    in the exact and the f64-FFT arithmetic; in fused mode also on a string that went put -> get -> put -> get."""
    text = "Park at Rest"
    for arith in (0, 1):
        sk = _server(ck, arith)
        try:
            for mode in (0, 1):
                sk.set_mode(mode)
                twin = ck.encrypt(text, 1, None, sk)
                once = sk.store_put(ck.encrypt(text, 1, None, sk))
                entries = [once]
                if mode == 1:
                    entries.append(sk.store_put(once.get()))
                    _, meta = entries[1].export()
                    assert np.array_equal(meta, np.full(4 * 13, 1 | 2 << 16, np.uint64))    # two packings inside
                for e in entries:
                    s = e.get()
                    where = (arith, mode, len(entries))
                    assert ck.decrypt(sk.to_upper(s)) == text.upper(), where
                    assert ck.decrypt_char(sk.contains_clear(s, "Rest")) == 1, where
                    assert ck.decrypt_char(sk.contains_clear(s, "rest")) == 0, where
                    assert ck.decrypt_char(sk.eq(s, twin)) == 1, where
                    assert ck.decrypt_char(sk.eq(e.get(), sk.to_upper(twin))) == 0, where
                    assert ck.decrypt_char(sk.find(s, ck.encrypt_no_padding("at", sk))) == 5, where
                    assert ck.decrypt_char(sk.find(e.get(3), ck.encrypt_no_padding("at", sk))) == 2, where   # a window
                    assert ck.decrypt(s) == text, where
                for e in entries:
                    e.drop()
            assert sk.store_stats()["device_bytes"] == 0
        finally:
            sk.close()


def test_noise_figures_and_rotation_groups(ck):
    """The planner cases of tests/test_store.py on real ciphertexts: x + 1 and x + 2 in fused mode share one blind rotation
    per block 0, their sum is charged 4 -- also restored, also from two separate get calls, also restored against
    original --, export renumbers the group to 1 and an import of those bytes keeps its members together; declared
    figures and the cycle limit hold; every sum decrypts."""
    from fhestring_amd.api import FheString, store_export_from_bytes, store_export_to_bytes
    sk = _server(ck, 1)
    try:
        def add_cost(p, q, want):
            sk.stats(reset=True)
            r = p.add(q)
            sk.flush()
            assert ck.decrypt_char(r) == want
            return sk.stats()["max_input_sum_c2"]

        x, y = ck.encrypt("ab", 0, None, sk).chars
        y.set_noise(9)
        r1, r2 = x.add(sk.trivial(1)), x.add(sk.trivial(2))
        sk.flush()
        assert sk.stats()["pbs_extracted"] >= 1
        vx, v1, v2 = ord("a"), ord("a") + 1, ord("a") + 2
        assert add_cost(r1, r2, (v1 + v2) & 255) == 4
        e = sk.store_put(FheString([r1, r2, y]))
        both = e.get()
        assert [h.sum_c2() for h in both.chars] == [1, 1, 9]
        assert add_cost(both[0], both[1], (v1 + v2) & 255) == 4
        first, second = e.get(0, 1)[0], e.get(1, 1)[0]
        assert add_cost(first, second, (v1 + v2) & 255) == 4 and add_cost(first, r2, (v1 + v2) & 255) == 4
        assert add_cost(first, x, (v1 + vx) & 255) == 3                           # strangers: 2, and the carry block's 3
        compact, meta = e.export()
        assert [int(m) >> 32 for m in meta[:8:4]] == [1, 1] and not (meta[1:4] >> np.uint64(32)).any()
        assert [int(m) & 0xffff for m in meta[8:]] == [9] * 4 and {int(m) >> 16 & 0xff for m in meta} == {1}
        data = store_export_to_bytes(compact, meta)
        imp = sk.store_import(*store_export_from_bytes(data))
        got, meta2 = imp.export()
        assert got.to_bytes() == compact.to_bytes() and np.array_equal(meta2, meta)
        p, q, z = imp.get().chars
        assert np.array_equal(FheString([p, q, z]).download(), both.download())   # the same words, restored the same way
        assert add_cost(p, q, (v1 + v2) & 255) == 4 and add_cost(p, second, (v1 + v2) & 255) == 3 and z.sum_c2() == 9
        # the cycle limit on the device, through the export format: 15 more packings may follow the first, not 16
        s = imp.get()
        for cycle in range(2, 17):
            en = sk.store_put(s)
            s = en.get()
            en.drop()
        assert _put_code(sk, s) == FHS_ERR_LIMIT
        assert ck.decrypt_str_raw(s.download()) == chr(v1) + chr(v2) + "b"        # sixteen packings deep and still exact
        assert _put_code(sk, sk.to_upper(s)) == FHS_ERR_LIMIT                     # fused: the character's own blocks are not bootstrapped
        sk.set_mode(0)
        assert _put_code(sk, sk.to_upper(s)) == 0                                 # as written: every block is a bootstrap output
    finally:
        sk.close()


def test_import_of_a_public_key_string(ck):
    """A public-key encrypted string parked as it arrives (meta=None) and read back, whole and by window, is bit-equal to
    upload_compact_string of the same bytes; it needs neither a packing key nor an expansion of the whole string."""
    pp = ck.get_public_parameters()
    pp.set_insecure_seed(77)
    rng = np.random.default_rng(10)
    text = "".join(chr(c) for c in rng.integers(32, 127, 600))
    c = pp.encrypt(text, 3)
    sk = _server(ck, 1, packing_key=False)
    try:
        before = sk.stats()["blocks_live"]
        e = sk.store_import(c)
        assert sk.stats()["blocks_live"] == before and len(e) == 603 and e.device_bytes == c.nbytes - 16
        got, meta = e.export()
        assert got.to_bytes() == c.to_bytes() and np.array_equal(meta, np.ones(4 * 603, np.uint64))
        assert np.array_equal(e.get().download(), sk.upload_compact_string(c).download())
        assert np.array_equal(e.get(509, 6).download(), sk.upload_compact_string(c, 509, 6).download())
        s = e.get(100, 64)
        assert [h.sum_c2() for h in s.chars] == [1] * 64
        assert ck.decrypt_char(sk.contains_clear(s, text[120:126])) == 1
        assert _put_code(sk, s) == FHS_ERR_STATE                                  # no packing key: put refuses, get worked
    finally:
        sk.close()
        pp.close()


def test_states_and_lifetime(ck):
    sk = _server(ck, 1)
    try:
        L, h = sk.ctx._L, sk.ctx._h
        before = sk.stats()["blocks_live"]
        s = ck.encrypt("at rest", 1, None, sk)
        assert sk.stats()["blocks_live"] == before + 32
        e = sk.store_put(s)
        del s
        assert sk.stats()["blocks_live"] == before                                # the pool blocks are back, the entry stays
        assert sk.store_stats() == {"entries": 1, "chars": 8, "device_bytes": 8192 + 128}
        hs = (C.c_uint64 * 4)()
        assert L.fhs_store_get(h, e.id, 7, 2, hs) == FHS_ERR_ARG and L.fhs_store_get(h, e.id + 1, 0, 1, hs) == FHS_ERR_ARG
        sk.ctx.load_server_key(ck.bsk(), ck.ksk())                                # entries survive; the packing key does not
        back = e.get()
        assert ck.decrypt(back) == "at rest" and ck.decrypt(sk.to_upper(back)) == "AT REST"
        assert _put_code(sk, back) == FHS_ERR_STATE
        sk.load_packing_key(ck)
        e2 = sk.store_put(back)
        assert e2.id != e.id and ck.decrypt(e2.get()) == "at rest"
        e.drop()
        assert L.fhs_store_drop(h, e.id) == FHS_ERR_ARG and L.fhs_store_get(h, e.id, 0, 1, hs) == FHS_ERR_ARG
        e2.drop()
        assert sk.store_stats() == {"entries": 0, "chars": 0, "device_bytes": 0}
        sk.store_put(back)                                                        # close() with a live entry is clean
        assert sk.store_stats()["entries"] == 1
    finally:
        sk.close()
    assert sk.ctx._h is None
