"""Fetching a row of a parked table by encrypted index, on the host (include/fhestring_hip.h, "fetching a row by encrypted
index"): the host reference against a numpy restatement of the formulas that uses no transform,
decryption of every row of the shapes the device test runs with the derived noise, the query, and the bookkeeping on a
planner context.  The device kernel is compared with the host reference, word for word, in _smoke_select of
__graft_entry__.py (tests/test_select_device.py)."""
import concurrent.futures
import ctypes as C
import math
import os

import numpy as np
import pytest

from ring_util import digits32, glwe_phases, negacyclic, round32

N = 2048
GLWE_NOISE = 2.9403601535432533e-16          # client.cpp: GLWE noise as a fraction of the torus
FHS_ERR_ARG, FHS_ERR_STATE, FHS_ERR_LIMIT = -1, -3, -4
CHOSEN = (0x00000000, 0x00008000, 0x7FFF8000, 0x80000000, 0xFFFFFFFF, 0x00007FFF)   # _smoke_rekey's digit boundaries
SHAPES = ((2, 1), (512, 1), (1536, 512), (640, 128), (2624, 64))                    # (n_chars, row_chars)
U64 = np.uint64


def _geometry(n_chars, row_chars):
    """(groups, row_blocks, rotate bits, tree levels) as the header states them"""
    rows, groups, row_blocks = n_chars // row_chars, (4 * n_chars + N - 1) // N, 4 * row_chars
    bits = (rows - 1).bit_length()
    rot = bits if groups == 1 else (512 // row_chars).bit_length() - 1
    return groups, row_blocks, rot, bits - rot


def _np_cmux(ggsw, a, b):
    """the header's one CMux: a, b = (mask32[N], body32[N]); ggsw [4][mask, body][N] raw words"""
    K = (ggsw + U64(32)) & ~U64(63)                                  # round_to_grid(., 6)
    d = digits32(b[0] - a[0]) + digits32(b[1] - a[1])                # mask d_0, mask d_1, body d_0, body d_1
    for x, dd in ((b[0] - a[0], d[:2]), (b[1] - a[1], d[2:])):
        assert np.array_equal(dd[0].view(U64) << U64(48), (x.astype(U64) << U64(32)) - (dd[1].view(U64) << U64(32)))
    out = []
    for col in range(2):
        s = sum((negacyclic(d[l], K[l, col]) for l in range(4) if d[l].any()), np.zeros(N, U64))
        out.append(round32((a[col].astype(U64) << U64(32)) + s))
    return out


def _np_select(query, mask32, body32, n_chars, row_chars):
    groups, row_blocks, rot, levels = _geometry(n_chars, row_chars)
    body = np.zeros(groups * N, np.uint32)
    body[:4 * n_chars] = body32                                      # words an entry does not store count as 0
    level = [(mask32[g], body[g * N:(g + 1) * N]) for g in range(groups)]
    zero = (np.zeros(N, np.uint32), np.zeros(N, np.uint32))
    for t in range(levels):
        level = [_np_cmux(query[rot + t], level[2 * i], level[2 * i + 1] if 2 * i + 1 < len(level) else zero)
                 for i in range((len(level) + 1) // 2)]
    g = level[0]
    for k in range(rot):
        s = row_blocks << k
        sign = np.where(np.arange(N) + s >= N, -1, 1).astype(np.int64).astype(np.uint32)
        g = _np_cmux(query[k], g, [np.roll(x, -s) * sign for x in g])
    return g[0], g[1][:row_blocks]


@pytest.fixture(scope="module")
def client():
    from fhestring_amd.api import MyClientKey
    a = MyClientKey(0xA11CE)
    yield a
    a.close()


@pytest.fixture()
def sk():
    from fhestring_amd.api import MyServerKey
    s = MyServerKey.planner()
    s.set_auto_flush(0)
    yield s
    s.close()


def test_host_reference_equals_schoolbook_in_every_word(client):
    from fhestring_amd.api import select_bits, select_host
    n_chars, row_chars = 1536, 256                                   # 3 groups, r = 1: two tree levels (a null sibling), one rotate
    assert select_bits(n_chars, row_chars) == 3 and _geometry(n_chars, row_chars) == (3, 1024, 1, 2)
    rng = np.random.default_rng(23)
    entries = []
    for chosen in (False, True):
        mask = rng.integers(0, 1 << 32, (3, N), dtype=np.uint32)
        if chosen:                                                   # differences of these meet the digit boundaries too
            mask[:] = rng.choice(np.array(CHOSEN, np.uint32), (3, N))
        entries.append((mask, rng.integers(0, 1 << 32, 4 * n_chars, dtype=np.uint32)))
    for index in range(8):                                           # 6 and 7 name no row: deterministic all the same
        query, bits = client.select_query(index, n_chars, row_chars)
        assert bits == 3 and query.shape == (3, 4, 2, N)
        for mask, body in entries:
            want = _np_select(query, mask, body, n_chars, row_chars)
            got = select_host(query, mask, body, 4 * n_chars, row_chars)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), index
            again = select_host(query, mask, body, 4 * n_chars, row_chars)
            assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), index
    # a query off the grid: the reference rounds it first, as the re-key reference rounds its key
    query = rng.integers(0, 1 << 64, (3, 4, 2, N), dtype=U64)
    want = _np_select(query, *entries[1], n_chars, row_chars)
    got = select_host(query, *entries[1], 4 * n_chars, row_chars)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _derived_sigma(n_cmux, s_weight):
    """per CMux the external product, 4 x 2048 digits of variance 2^32 / 12 on key rows of the GLWE
    noise, and the 32-bit rounding of mask and body"""
    s_glwe = GLWE_NOISE * 2.0 ** 64
    return math.sqrt(n_cmux * (4 * N * 2.0 ** 32 / 12 * s_glwe ** 2 + 2.0 ** 64 / 12 * (1 + s_weight)))


@pytest.mark.parametrize("n_chars,row_chars", SHAPES)
def test_every_row_decrypts_with_the_derived_noise(client, n_chars, row_chars):
    from fhestring_amd.api import SELECT_REKEY_COST, select_host
    groups, row_blocks, rot, levels = _geometry(n_chars, row_chars)
    rows = n_chars // row_chars
    text = "".join(chr(33 + (7 * i + i // row_chars) % 90) for i in range(n_chars))
    pa = client.get_public_parameters()
    pa.set_insecure_seed(7 + n_chars)
    c = pa.encrypt(text, 0)                                          # the compact format of an entry, without a GPU
    pa.close()
    s = client.secret_keys()[1]
    source = [glwe_phases(c.mask32[g].astype(U64) << U64(32), U64(0), s) for g in range(groups)]
    body = np.zeros(groups * N, np.uint32)
    body[:4 * n_chars] = c.body32
    source = np.concatenate(source) + (body.astype(U64) << U64(32))

    def one_row(p):
        query, bits = client.select_query(p, n_chars, row_chars)
        row = select_host(query, c, row_chars=row_chars)
        assert len(row) == row_chars and row.mask32.shape == (1, N)
        assert client.decrypt_str_raw(row.expand()) == text[p * row_chars:(p + 1) * row_chars], p
        if p % max(1, rows // 8) and p != rows - 1:                  # the noise of some rows, first and last among them
            return None
        ph = glwe_phases(row.mask32[0].astype(U64) << U64(32), U64(0), s)[:row_blocks] + (row.body32.astype(U64) << U64(32))
        return (ph - source[p * row_blocks:(p + 1) * row_blocks]).view(np.int64).astype(np.float64)

    # (the library calls release the interpreter lock and a query has streams of its own: rows go side by side)
    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        added = [a for a in pool.map(one_row, range(rows)) if a is not None]
    added = np.concatenate(added)
    derived = _derived_sigma(levels + rot, float(s.sum()))
    sigma = float(added.std())
    print("select (%d, %d): %d CMuxes, added sigma 2^%.2f, derived 2^%.2f, max |e| 2^%.2f" %
          (n_chars, row_chars, levels + rot, math.log2(sigma), math.log2(derived), math.log2(np.abs(added).max())))
    assert derived / 2 < sigma < derived * 2
    assert np.abs(added).max() < 2.0 ** 46
    # the charge: FHS_SELECT_REKEY_COST re-keys per CMux cover it (the header's 2^32.6 and 2^35.2 of one re-key)
    rekey_var = 2 * N * 2.0 ** 32 / 12 * (GLWE_NOISE * 2.0 ** 64) ** 2 + 2.0 ** 64 / 12 * (1 + float(s.sum()))
    assert derived ** 2 <= SELECT_REKEY_COST * (levels + rot) * rekey_var and SELECT_REKEY_COST == 2


def test_an_index_past_the_table_gives_nul_where_nodes_are_missing(client):
    from fhestring_amd.api import select_host
    n_chars, row_chars = 1536, 512                                   # 3 groups = 3 rows, 2 bits: index 3 names the missing node
    pa = client.get_public_parameters()
    pa.set_insecure_seed(5)
    c = pa.encrypt("x" * n_chars, 0)
    pa.close()
    query, _ = client.select_query(3, n_chars, row_chars)
    row = select_host(query, c, row_chars=row_chars)
    assert client.decrypt_str_raw(row.expand()) == ""


def _row_error(row, s, bit, l, mask_row):
    """body - mask (*) S - m of one GGSW row as signed words; m = bit (-S) g_l for a mask-digit row, bit g_l otherwise"""
    g = U64(1) << U64(64 - 16 * (l + 1))
    m = (U64(0) - s * g) if mask_row else np.where(np.arange(N) == 0, g, U64(0))
    return (row[1] - negacyclic(s.astype(np.int64), row[0]) - U64(bit) * m).view(np.int64)


def test_query(client):
    from fhestring_amd.api import MyClientKey, SELECT_QUERY_BIT_WORDS
    s = client.secret_keys()[1]
    n_chars, row_chars = 640, 128                                    # 3 bits
    q1, bits = client.select_query(5, n_chars, row_chars)
    q2, _ = client.select_query(5, n_chars, row_chars)
    assert bits == 3 and q1.size == bits * SELECT_QUERY_BIT_WORDS == 3 * 4 * 2 * N and not (q1 & U64(63)).any()   # the 58-bit grid
    for q in (q1, q2):
        for k in range(bits):
            for r in range(4):
                assert np.abs(_row_error(q[k, r], s, (5 >> k) & 1, r & 1, r < 2)).max() < 2 ** 18, (k, r)
    assert np.abs(_row_error(q1[0, 2], s, 0, 0, False)).max() > 2 ** 40                   # (bit 0 of 5 is set)
    assert np.abs(_row_error(q1[1, 0], s, 1, 0, True)).max() > 2 ** 40                    # (bit 1 is not)
    masks = lambda q: q[:, :, 0]
    q3, _ = client.select_query(2, n_chars, row_chars)
    fresh = MyClientKey()
    try:
        q4, _ = fresh.select_query(5, n_chars, row_chars)
        q5, _ = fresh.select_query(5, n_chars, row_chars)
        sf = fresh.secret_keys()[1]
        assert np.abs(_row_error(q4[2, 3], sf, 1, 1, False)).max() < 2 ** 18
    finally:
        fresh.close()
    every = [masks(q) for q in (q1, q2, q3, q4, q5)]
    assert all((every[i] == every[j]).mean() < 0.01 for i in range(5) for j in range(i)), "two queries share a mask"
    noise = [np.stack([_row_error(q[k, 2], s, (5 >> k) & 1, 0, False) for k in range(3)]) for q in (q1, q2)]
    assert (noise[0] == noise[1]).mean() < 0.01, "two queries for one index share their noise"
    # seeded clients reproduce: the n-th query of a fresh client with the same seed is the same words
    twin = MyClientKey(0xA11CE)
    other = MyClientKey(0xA11CF)
    try:
        first = MyClientKey(0xA11CE)
        try:
            want = [first.select_query(5, n_chars, row_chars)[0] for _ in range(2)]
        finally:
            first.close()
        got = [twin.select_query(5, n_chars, row_chars)[0] for _ in range(2)]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not np.array_equal(got[0], got[1])
        assert (masks(other.select_query(5, n_chars, row_chars)[0]) == masks(got[0])).mean() < 0.01
    finally:
        twin.close()
        other.close()
    L = client._L
    out = np.zeros(SELECT_QUERY_BIT_WORDS, U64)
    assert L.fhs_client_select_query(client._h, 0, 0, out.ctypes.data) == FHS_ERR_ARG
    assert L.fhs_client_select_query(client._h, 0, 25, out.ctypes.data) == FHS_ERR_ARG
    assert L.fhs_client_select_query(client._h, 0, 1, None) == FHS_ERR_ARG


def test_select_bits():
    from fhestring_amd.api import select_bits
    for (n, r), bits in zip(SHAPES + ((1536, 256), (1024, 512), (4096, 64)), (1, 9, 2, 3, 6, 3, 1, 6)):
        assert select_bits(n, r) == bits, (n, r)
    for n, r in ((6, 3), (2048, 1024), (6, 4), (4, 4), (0, 1), (8, 0), (512, 512)):      # not a power of two, > 512, not a
        assert select_bits(n, r) == 0, (n, r)                                           # multiple, one row, nothing


def test_bookkeeping_on_a_planner_context(sk):
    from fhestring_amd.api import FheString, SELECT_QUERY_BIT_WORDS, STORE_MAX_REKEYS, _harr
    L, h = sk.ctx._L, sk.ctx._h
    sk.set_mode(1)
    query = np.zeros(SELECT_QUERY_BIT_WORDS, U64)                   # a planner reads no word of it

    def add_cost(p, q):
        sk.stats(reset=True)
        r = p.add(q)
        sk.flush()
        return sk.stats()["max_input_sum_c2"] if r is not None else None

    def select_rc(eid, row_chars, bits, q=query):
        out = C.c_uint64(77)
        rc = L.fhs_store_select(h, eid, row_chars, None if q is None else q.ctypes.data, bits, C.byref(out))
        assert rc == 0 or out.value == 0
        return rc

    # figures and cycles: the maxima over the rows, block by block.  Rows (x, y) and (z, w): z carries figure 9, y figure 5,
    # and w comes out of another entry, so it has one packing more
    x, y, z, w0 = sk.dummy_string(4).chars
    z.set_noise(9)
    y.set_noise(5)
    t = sk.store_put(FheString([w0]))
    w = t.get()[0]
    e = sk.store_put(FheString([x, y, z, w]))
    entries = sk.store_stats()["entries"]
    sel = e.select(query, 2)
    assert sel.id not in (0, e.id, t.id) and len(sel) == 2 and sel.device_bytes == 4 * N + 4 * 8 and len(e) == 4
    assert sk.store_stats()["entries"] == entries + 1
    got = sel.get()
    assert [c.sum_c2() for c in got.chars] == [9, 5]
    assert e.rekeys == 0 and sel.rekeys == 2                          # one rotate bit, FHS_SELECT_REKEY_COST each
    # cycles: w's blocks were packed twice, so the result's second character has cycles 2 and its first 1: from there
    # 14 and 15 more put / get rounds pass
    for k, rounds in ((1, 14), (0, 15)):
        s = FheString([got[k]])
        for cycle in range(rounds):
            tt = sk.store_put(s)
            s = tt.get()
            tt.drop()
        eid = C.c_uint64(0)
        assert L.fhs_store_put(h, _harr(s.chars), 1, C.byref(eid)) == FHS_ERR_LIMIT, k
    # rotation groups: x + 1 and x + 2 share one blind rotation (tests/test_store.py): their sum costs 4, two strangers 3
    a, b, c, d = sk.dummy_string(4).chars
    r1, r2 = a.add(sk.trivial(1)), a.add(sk.trivial(2))
    sk.flush()
    assert add_cost(r1, r2) == 4 and add_cost(r1, b) == 3
    grouped = sk.store_put(FheString([r1, b, c, r2])).select(query, 2).get()     # each result character has one grouped candidate
    assert add_cost(grouped[0], grouped[1]) == 4                      # one fresh group shared by both: fully correlated
    mixed = sk.store_put(FheString([r1, b, c, d])).select(query, 2).get()        # only the first has one
    assert add_cost(mixed[0], mixed[1]) == 3
    plain = sk.store_put(FheString([b, c, d, b])).select(query, 2).get()         # no candidate has one
    assert add_cost(plain[0], plain[1]) == add_cost(b, c) < 4
    # the counter: source + FHS_SELECT_REKEY_COST x (tree levels + rotate bits), refused past FHS_STORE_MAX_REKEYS
    big = sk.store_put(sk.dummy_string(1280))                         # 3 groups; rows of 128: 2 rotate bits + 2 tree levels
    q4 = np.zeros(4 * SELECT_QUERY_BIT_WORDS, U64)
    assert big.select(q4, 128).rekeys == 8 and big.rekey().select(q4, 128).rekeys == 9
    assert STORE_MAX_REKEYS == 255
    for i in range(253 - e.rekeys):
        assert L.fhs_store_rekey(h, e.id, None) == 0
    assert e.rekeys == 253 and e.select(query, 2).rekeys == 255
    e.rekey()
    entries = sk.store_stats()["entries"]
    assert select_rc(e.id, 2, 1) == FHS_ERR_LIMIT and sk.store_stats()["entries"] == entries and e.rekeys == 254
    assert select_rc(e.id, 1, 2) == FHS_ERR_LIMIT                     # (two rotate bits: 258)
    # every refused shape, on an entry of 6 characters and on e (4 characters)
    six = sk.store_put(sk.dummy_string(6))
    assert select_rc(six.id, 3, 1) == FHS_ERR_ARG                     # not a power of two
    assert select_rc(six.id, 4, 1) == FHS_ERR_ARG                     # 6 is no multiple of 4
    assert select_rc(six.id, 1024, 1) == FHS_ERR_ARG and select_rc(big.id, 1024, 1) == FHS_ERR_ARG     # rows longer than a group
    assert select_rc(six.id, 0, 1) == FHS_ERR_ARG
    f = sk.store_put(sk.dummy_string(4))
    assert select_rc(f.id, 4, 1) == FHS_ERR_ARG and select_rc(f.id, 4, 0) == FHS_ERR_ARG            # one row
    assert select_rc(f.id, 2, 2) == FHS_ERR_ARG and select_rc(f.id, 2, 0) == FHS_ERR_ARG            # bits is 1
    assert select_rc(f.id, 1, 1) == FHS_ERR_ARG and select_rc(six.id, 2, 1) == FHS_ERR_ARG          # bits is 2
    assert select_rc(12345, 2, 1) == FHS_ERR_ARG and select_rc(0, 2, 1) == FHS_ERR_ARG              # unknown id
    assert select_rc(f.id, 2, 1, None) == FHS_ERR_ARG and L.fhs_store_select(h, f.id, 2, query.ctypes.data, 1, None) == FHS_ERR_ARG
    assert select_rc(f.id, 2, 1) == 0 and select_rc(six.id, 2, 2) == 0
    f.drop()
    assert select_rc(f.id, 2, 1) == FHS_ERR_ARG
    # a planner computes nothing: the diagnostic says so
    m, bb = np.zeros((1, N), np.uint32), np.zeros(8, np.uint32)
    assert L.fhs_debug_select_device(h, query.ctypes.data, 1, m.ctypes.data, bb.ctypes.data, 8, 1, m.ctypes.data,
                                     bb.ctypes.data) == FHS_ERR_STATE


def test_host_reference_refuses_what_the_store_refuses():
    import fhestring_amd
    L = fhestring_amd.lib()
    q = np.zeros(2 * 4 * 2 * N, U64)
    m, b, mo, bo = np.zeros((1, N), np.uint32), np.zeros(16, np.uint32), np.zeros(N, np.uint32), np.zeros(16, np.uint32)
    args = lambda n_blocks, row_chars, bits: (q.ctypes.data, bits, m.ctypes.data, b.ctypes.data, n_blocks, row_chars,
                                              mo.ctypes.data, bo.ctypes.data)
    assert L.fhs_store_select_host(*args(16, 2, 1)) == 0 and L.fhs_store_select_host(*args(16, 1, 2)) == 0
    for n_blocks, row_chars, bits in ((16, 2, 2), (16, 4, 1), (16, 3, 1), (14, 1, 2), (12, 2, 1), (16, 0, 1)):
        assert L.fhs_store_select_host(*args(n_blocks, row_chars, bits)) == FHS_ERR_ARG, (n_blocks, row_chars, bits)
    assert L.fhs_store_select_host(None, 1, m.ctypes.data, b.ctypes.data, 16, 2, mo.ctypes.data, bo.ctypes.data) == FHS_ERR_ARG
