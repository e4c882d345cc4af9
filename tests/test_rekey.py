"""Re-keying parked store entries to another client key, on the host (include/fhestring_hip.h, "re-keying parked
entries"): the host reference against a numpy restatement of the formulas that uses no transform,
decryption under the new key with the derived noise, the re-key key and its key file, and the bookkeeping on a planner
context.  The device kernel is compared with the host reference, word for word, in smoke() of __graft_entry__.py."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

from ring_util import block_phases, digits32, negacyclic, round32

N = 2048
BIG_CT = 2049
GLWE_NOISE = 2.9403601535432533e-16          # client.cpp: GLWE noise as a fraction of the torus
LEVELS, BASE_LOG = 2, 16
FHS_ERR_ARG, FHS_ERR_STATE, FHS_ERR_LIMIT = -1, -3, -4
HEADER_WORDS = (742, 2048, 5, 3, 23, 6)      # lwe_n, poly_n, ks_levels, ks_base_log, pbs_base_log, bsk_quant_bits
CHOSEN = (0x00000000, 0x00008000, 0x7FFF8000, 0x80000000, 0xFFFFFFFF, 0x00007FFF)
U64 = np.uint64


def _np_rekey(key, mask32, body32, n_blocks):
    """the issue's formulas, group by group"""
    K = ((key + U64(32)) & ~U64(63)).reshape(LEVELS, 2, N)        # round_to_grid(., 6)
    mask32 = mask32.reshape(-1, N)
    m_out, b_out = np.zeros_like(mask32), np.zeros(n_blocks, np.uint32)
    for g in range(mask32.shape[0]):
        count = min(N, n_blocks - g * N)
        d = digits32(mask32[g])
        A = mask32[g].astype(U64) << U64(32)
        assert np.array_equal(d[0].view(U64) << U64(48), A - (d[1].view(U64) << U64(32)))     # A = d_0 2^48 + d_1 2^32
        assert all(int(x.min()) >= -(1 << 15) and int(x.max()) < (1 << 15) for x in d)
        s = [sum((negacyclic(d[l], K[l, col]) for l in range(LEVELS)), np.zeros(N, U64)) for col in range(2)]
        m_out[g] = round32(U64(0) - s[0])
        b = body32[g * N:g * N + count].astype(U64) << U64(32)
        b_out[g * N:g * N + count] = round32(b - s[1][:count])
    return m_out, b_out


@pytest.fixture(scope="module")
def clients():
    from fhestring_amd.api import MyClientKey
    a, b = MyClientKey(0xA11CE), MyClientKey(0xB0B)
    yield a, b
    a.close()
    b.close()


@pytest.fixture()
def sk():
    from fhestring_amd.api import MyServerKey
    s = MyServerKey.planner()
    s.set_auto_flush(0)
    yield s
    s.close()


def test_host_reference_equals_schoolbook_in_every_word():
    import fhestring_amd
    from fhestring_amd.api import REKEY_KEY_WORDS, rekey_host
    rng = np.random.default_rng(14)
    key = rng.integers(0, 1 << 64, REKEY_KEY_WORDS, dtype=U64)     # off the grid: the reference rounds it first
    for n_blocks in (1, 24, 2048, 2052):
        g = (n_blocks + N - 1) // N
        mask = rng.integers(0, 1 << 32, (g, N), dtype=np.uint32)
        body = rng.integers(0, 1 << 32, n_blocks, dtype=np.uint32)
        want = _np_rekey(key, mask, body, n_blocks)
        got = rekey_host(key, mask, body, n_blocks)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), n_blocks
        m2, b2 = mask.copy(), body.copy()                            # aliased output = separate output
        assert fhestring_amd.lib().fhs_rekey_host(key.ctypes.data, m2.ctypes.data, b2.ctypes.data, n_blocks,
                                                  m2.ctypes.data, b2.ctypes.data) == 0
        assert np.array_equal(m2, want[0]) and np.array_equal(b2, want[1]), n_blocks
    # digit boundaries and the carry out of the top digit: about 2^-16 per random word, so they are chosen
    body = rng.integers(0, 1 << 32, N, dtype=np.uint32)
    for word in CHOSEN:
        mask = np.full((1, N), word, np.uint32)
        want = _np_rekey(key, mask, body, N)
        got = rekey_host(key, mask, body, N)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), hex(word)
        if word == 0:
            assert not got[0].any() and np.array_equal(got[1], body)
    mixed = rng.choice(np.array(CHOSEN, np.uint32), (1, N))          # ... and all of them in one polynomial
    want = _np_rekey(key, mixed, body, 777)
    got = rekey_host(key, mixed, body[:777], 777)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_it_decrypts_under_the_new_key_with_the_derived_noise(clients):
    from fhestring_amd.api import rekey_host
    a, b = clients
    text = "".join(chr(33 + (7 * i) % 90) for i in range(513))       # two groups, the second with 4 bodies
    pa = a.get_public_parameters()
    pa.set_insecure_seed(99)
    c = pa.encrypt(text, 0)                                          # fhs_public_encrypt_str
    pa.close()
    assert len(c) == 513 and c.mask32.shape == (2, N)
    c2 = rekey_host(a.rekey_key(b), c)
    before, after = c.expand(), c2.expand()
    assert b.decrypt_str_raw(after) == text and a.decrypt_str_raw(before) == text
    try:
        wrong = a.decrypt_str_raw(after)
    except UnicodeDecodeError:                                       # not even ASCII
        wrong = None
    assert wrong != text
    sa, sb = a.secret_keys()[1], b.secret_keys()[1]
    added = (block_phases(after, sb) - block_phases(before, sa)).view(np.int64).astype(np.float64)
    s_glwe = GLWE_NOISE * 2.0 ** 64
    derived = math.sqrt(LEVELS * N * 2.0 ** 32 / 12 * s_glwe ** 2 + 2.0 ** 64 / 12 * (1 + float(sb.sum())))
    sigma = float(added.std())
    print("re-key: added sigma 2^%.2f, derived 2^%.2f, max |e| 2^%.2f" %
          (math.log2(sigma), math.log2(derived), math.log2(np.abs(added).max())))
    assert derived / 2 < sigma < derived * 2
    assert np.abs(added).max() < 2.0 ** 40


def _key_error(key, s_from, s_to):
    """body - mask (*) S_to - S_from 2^(64 - 16 (l + 1)) of every level, as signed words"""
    K = key.reshape(LEVELS, 2, N)
    out = []
    for l in range(LEVELS):
        e = K[l, 1] - negacyclic(s_to.astype(np.int64), K[l, 0]) - (s_from << U64(64 - BASE_LOG * (l + 1)))
        out.append(e.view(np.int64))
    return np.stack(out)


def test_key_and_key_file(clients, sk, tmp_path):
    import fhestring_amd
    from fhestring_amd import cabi
    from fhestring_amd.api import MyClientKey, REKEY_KEY_WORDS
    a, b = clients
    sa, sb = a.secret_keys()[1], b.secret_keys()[1]
    k1, k2 = a.rekey_key(b), a.rekey_key(b)
    for k in (k1, k2):
        assert k.size == REKEY_KEY_WORDS == 2 * 2 * N and not (k & U64(63)).any()            # on the 58-bit grid
        assert np.abs(_key_error(k, sa, sb)).max() < 2 ** 18
    assert np.abs(_key_error(k1, sb, sa)).max() > 2 ** 40                                     # (the direction matters)
    masks = lambda k: k.reshape(LEVELS, 2, N)[:, 0]
    assert not np.array_equal(masks(k1), masks(k2))                   # fresh randomness per call, seeded clients too
    c, fresh = MyClientKey(0xC0C0A), MyClientKey()
    try:
        k3, k4, k5 = c.rekey_key(b), a.rekey_key(fresh), a.rekey_key(fresh)
        sf = fresh.secret_keys()[1]
        assert np.abs(_key_error(k4, sa, sf)).max() < 2 ** 18
    finally:
        c.close()
        fresh.close()
    every = [masks(k) for k in (k1, k2, k3, k4, k5)]
    assert all((every[i] == every[j]).mean() < 0.01 for i in range(5) for j in range(i)), "two re-key keys share a mask"
    # kind 7 file.  Seeded clients are reproducible: the first key of a fresh pair with the same seeds is the file's payload.
    consts = dict(cabi.parse_header()["consts"])
    path = str(tmp_path / "kind7.key")
    a2, b2, a3, b3 = (MyClientKey(s) for s in (0xA11CE, 0xB0B, 0xA11CE, 0xB0B))
    try:
        first = a2.rekey_key(b2)
        a3.save_rekey_key(b3, path)
    finally:
        for k in (a2, b2, a3, b3):
            k.close()
    assert os.path.getsize(path) == consts["FHS_REKEY_KEY_FILE_BYTES"] == 64 + 8 * REKEY_KEY_WORDS == 64 + 65536
    data = open(path, "rb").read()
    assert data[:64] == b"FHSKEY01" + struct.pack("<7Q", 7, *HEADER_WORDS)
    assert data[64:] == first.tobytes()
    assert np.abs(_key_error(np.frombuffer(data, U64, REKEY_KEY_WORDS, 64), sa, sb)).max() < 2 ** 18

    L, h = fhestring_amd.lib(), sk.ctx._h

    def refused(loader, p):
        rc = getattr(L, loader)(h, p.encode())
        return rc == FHS_ERR_STATE and L.fhs_last_error(h).startswith(b"cannot read")

    assert not refused("fhs_load_rekey_key_file", path)
    for delta, what in ((b"\0", "one byte more"), (None, "one byte less")):
        p = str(tmp_path / "resized.key")
        open(p, "wb").write(data + delta if delta else data[:-1])
        assert refused("fhs_load_rekey_key_file", p), what
    # every loader of kinds 1-6 refuses the kind 7 file ...
    for loader in ("fhs_load_server_key_file", "fhs_load_multibit_key_file", "fhs_load_compressed_server_key_file",
                   "fhs_load_packing_key_file"):
        assert refused(loader, path), loader
    out = C.c_void_p()
    assert L.fhs_client_load(path.encode(), C.byref(out)) != 0 and not out.value
    assert L.fhs_public_key_load(path.encode(), C.byref(out)) != 0 and not out.value
    # ... and the new loader refuses kinds 1-6: the same payload and size under another kind, so the kind alone decides
    for kind in range(1, 7):
        p = str(tmp_path / ("as_kind%d.key" % kind))
        open(p, "wb").write(b"FHSKEY01" + struct.pack("<7Q", kind, *HEADER_WORDS) + data[64:])
        assert refused("fhs_load_rekey_key_file", p), kind
    open(p, "wb").write(b"FHSKEY01" + struct.pack("<7Q", 7, *HEADER_WORDS) + data[64:])
    assert not refused("fhs_load_rekey_key_file", p)


def test_bookkeeping_on_a_planner_context(sk):
    from fhestring_amd.api import CompactFheString, FheString, STORE_MAX_REKEYS, store_meta_word
    L, h = sk.ctx._L, sk.ctx._h
    sk.set_mode(1)

    def add_cost(p, q):
        sk.stats(reset=True)
        r = p.add(q)                                                 # (kept: a dropped handle takes its work with it)
        sk.flush()
        return sk.stats()["max_input_sum_c2"] if r is not None else None

    # x + 1 and x + 2 share one blind rotation (tests/test_store.py): their sum costs 4, two strangers 3
    x, y, z = sk.dummy_string(3).chars
    z.set_noise(9)
    r1, r2 = x.add(sk.trivial(1)), x.add(sk.trivial(2))
    sk.flush()
    e = sk.store_put(FheString([r1, r2, y, z]))
    figures = [c.sum_c2() for c in e.get().chars]
    info = (len(e), e.device_bytes)
    assert e.rekeys == 0 and figures[3] == 9
    assert e.rekey() is e and e.rekeys == 1                         # in place: a planner needs no key
    assert (len(e), e.device_bytes) == info and sk.store_stats()["entries"] == 1
    back = e.get()
    assert [c.sum_c2() for c in back.chars] == figures
    assert add_cost(back[0], back[1]) == 4 and add_cost(back[0], back[2]) == 3 and add_cost(back[0], r2) == 4
    # cycles are untouched: the entry's blocks carry one packing, so 15 more put / get rounds pass and the 17th put is refused
    s = back
    for cycle in range(15):
        t = sk.store_put(s)
        s = t.get()
        t.drop()
    eid = C.c_uint64(0)
    from fhestring_amd.api import _harr
    assert L.fhs_store_put(h, _harr(s.chars), len(s.chars), C.byref(eid)) == FHS_ERR_LIMIT
    # a copy: a fresh id, the original as it was
    f = sk.store_put(FheString([r1, r2]))
    g = f.rekey(copy=True)
    assert g.id not in (0, e.id, f.id) and f.rekeys == 0 and g.rekeys == 1 and len(g) == len(f) == 2
    assert g.device_bytes == f.device_bytes and sk.store_stats()["entries"] == 3
    gb = g.get()
    assert add_cost(gb[0], gb[1]) == 4 and add_cost(gb[0], f.get(1, 1)[0]) == 4
    g2 = g.rekey(copy=True)
    assert g2.rekeys == 2 and g.rekeys == 1
    # errors
    out, n = C.c_uint64(77), C.c_uint32(0)
    assert L.fhs_store_rekey(h, 12345, None) == FHS_ERR_ARG
    assert L.fhs_store_rekey(h, 12345, C.byref(out)) == FHS_ERR_ARG and out.value == 0
    assert L.fhs_store_rekey(h, 0, None) == FHS_ERR_ARG and L.fhs_store_rekey_count(h, 12345, C.byref(n)) == FHS_ERR_ARG
    f.drop()
    assert L.fhs_store_rekey(h, f.id, None) == FHS_ERR_ARG
    # 255 re-keys of one entry succeed, the 256th is refused, in place and as a copy; nothing else changes
    assert STORE_MAX_REKEYS == 255
    for i in range(1, 255):
        assert L.fhs_store_rekey(h, e.id, None) == 0, i
    assert e.rekeys == 255
    entries = sk.store_stats()["entries"]
    assert L.fhs_store_rekey(h, e.id, None) == FHS_ERR_LIMIT
    assert L.fhs_store_rekey(h, e.id, C.byref(out)) == FHS_ERR_LIMIT and out.value == 0
    assert e.rekeys == 255 and sk.store_stats()["entries"] == entries
    assert [c.sum_c2() for c in e.get().chars] == figures
    # an imported entry starts at 0, whatever its meta words say about cycles
    c = CompactFheString(2, np.zeros((1, N), np.uint32), np.zeros(8, np.uint32))
    imp = sk.store_import(c, np.full(8, store_meta_word(3, 5, 1), U64))
    assert imp.rekeys == 0 and sk.store_import(c).rekeys == 0
    assert imp.rekey().rekeys == 1
    # a planner notes a key and converts nothing; unloading is allowed too
    sk.load_rekey_key(np.zeros(2 * 2 * N, U64))
    sk.load_rekey_key(None)
