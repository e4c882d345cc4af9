"""Seeded select queries and several queries per call, on the host (include/fhestring_hip.h, "seeded queries, queries
converted on the GPU, several queries per call"): the expansion of a seeded query selects every row
through the host reference, its masks depend on the seed alone, its noise is the GLWE noise and comes from streams of
its own, and a planner context books a seeded or batched call as it books the single calls.  The device side is
tests/test_select_seeded_device.py."""
import concurrent.futures
import ctypes as C
import os

import numpy as np
import pytest

from ring_util import negacyclic

N = 2048
GLWE_NOISE = 2.9403601535432533e-16          # client.cpp: GLWE noise as a fraction of the torus
FHS_ERR_ARG, FHS_ERR_LIMIT = -1, -4
U64 = np.uint64


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


@pytest.mark.parametrize("n_chars,row_chars", ((2, 1), (640, 128), (2624, 64)))
def test_every_row_is_selected_by_the_expanded_seeded_query(client, n_chars, row_chars):
    from fhestring_amd.api import SeededSelectQuery, expand_select_query, select_bits, select_host
    rows = n_chars // row_chars
    text = "".join(chr(33 + (5 * i + i // row_chars) % 90) for i in range(n_chars))
    pa = client.get_public_parameters()
    pa.set_insecure_seed(11 + n_chars)
    c = pa.encrypt(text, 0)
    pa.close()

    def one_row(p):
        q = client.select_query(p, n_chars, row_chars, seeded=True)
        assert isinstance(q, SeededSelectQuery) and q.bits == select_bits(n_chars, row_chars)
        assert q.seed.shape == (8,) and q.bodies.shape == (q.bits, 4, N)
        row = select_host(expand_select_query(q), c, row_chars=row_chars)
        assert client.decrypt_str_raw(row.expand()) == text[p * row_chars:(p + 1) * row_chars], p

    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(one_row, range(rows)))


def test_masks_come_from_the_seed_alone_and_bodies_are_copied(client):
    from fhestring_amd.api import SeededSelectQuery, expand_select_query
    q = client.select_query(5, 640, 128, seeded=True)
    full = expand_select_query(q)
    assert full.shape == (3, 4, 2, N)
    assert np.array_equal(full[:, :, 1], q.bodies), "a body changed on the way"
    blank = expand_select_query(SeededSelectQuery(q.seed, np.zeros_like(q.bodies), q.bits))
    assert np.array_equal(blank[:, :, 0], full[:, :, 0]) and not blank[:, :, 1].any()
    assert not (full[:, :, 0] & U64(63)).any(), "a mask word off the 58-bit grid"
    assert not (q.bodies & U64(63)).any()
    other = SeededSelectQuery(q.seed ^ np.array([1, 0, 0, 0, 0, 0, 0, 0], np.uint32), q.bodies, q.bits)
    assert (expand_select_query(other)[:, :, 0] == full[:, :, 0]).mean() < 0.01
    rows = full[:, :, 0].reshape(12, N)                              # every row a stream of its own
    assert all((rows[i] == rows[j]).mean() < 0.01 for i in range(12) for j in range(i))
    # the header's convention, restated: row r of bit k is stream 4k + r of domain 8, draws & ~63
    L = client._L
    nonce = (C.c_uint32 * 3)(8, 4 * 2 + 3, 0)
    draws = np.zeros(N, U64)
    L.fhs_chacha20_stream(q.seed.ctypes.data, 0, nonce, draws.ctypes.data, N)
    assert np.array_equal(full[2, 3, 0], draws & ~U64(63))
    out = np.zeros((1, 4, 2, N), U64)
    assert L.fhs_expand_select_query(None, q.bodies.ctypes.data, 1, out.ctypes.data) == FHS_ERR_ARG
    assert L.fhs_expand_select_query(q.seed.ctypes.data, None, 1, out.ctypes.data) == FHS_ERR_ARG
    assert L.fhs_expand_select_query(q.seed.ctypes.data, q.bodies.ctypes.data, 0, out.ctypes.data) == FHS_ERR_ARG
    assert L.fhs_expand_select_query(q.seed.ctypes.data, q.bodies.ctypes.data, 1, None) == FHS_ERR_ARG
    assert L.fhs_client_select_query_seeded(client._h, 0, 25, q.seed.ctypes.data, q.bodies.ctypes.data) == FHS_ERR_ARG
    assert L.fhs_client_select_query_seeded(client._h, 0, 1, None, q.bodies.ctypes.data) == FHS_ERR_ARG
    assert L.fhs_client_select_query_seeded(client._h, 0, 1, q.seed.ctypes.data, None) == FHS_ERR_ARG


def _row_error(row, s, bit, l, mask_row):
    """body - mask (*) S - m of one GGSW row as signed words (tests/test_select.py measures its rows the same way)"""
    g = U64(1) << U64(64 - 16 * (l + 1))
    m = (U64(0) - s * g) if mask_row else np.where(np.arange(N) == 0, g, U64(0))
    return (row[1] - negacyclic(s.astype(np.int64), row[0]) - U64(bit) * m).view(np.int64)


def test_phase_noise_and_freshness(client):
    from fhestring_amd.api import MyClientKey, expand_select_query
    s = client.secret_keys()[1]
    n_chars, row_chars, index = 640, 128, 5
    sigma = GLWE_NOISE * 2.0 ** 64
    q1 = client.select_query(index, n_chars, row_chars, seeded=True)
    errors = []
    f1 = expand_select_query(q1)
    for k in range(q1.bits):
        for r in range(4):
            e = _row_error(f1[k, r], s, (index >> k) & 1, r & 1, r < 2)
            errors.append(e)
            got = float(e.astype(np.float64).std())
            print("seeded query bit %d row %d: phase error sigma %.1f, GLWE noise %.1f" % (k, r, got, sigma))
            assert sigma / 2 < got < sigma * 2, (k, r)
    # noise streams are per call, bit and row: no two rows share their errors
    assert all((errors[i] == errors[j]).mean() < 0.01 for i in range(len(errors)) for j in range(i))
    # an entropy client: two queries for one index differ in seed and in every body row
    fresh = MyClientKey()
    try:
        a, b = (fresh.select_query(index, n_chars, row_chars, seeded=True) for _ in range(2))
        assert not np.array_equal(a.seed, b.seed)
        assert all((a.bodies[k, r] == b.bodies[k, r]).mean() < 0.01 for k in range(a.bits) for r in range(4))
        sf = fresh.secret_keys()[1]
        fa, fb = expand_select_query(a), expand_select_query(b)
        ea, eb = (_row_error(f[0, 2], sf, index & 1, 0, False) for f in (fa, fb))
        assert np.abs(ea).max() < 2 ** 18 and (ea == eb).mean() < 0.01, "two queries share their noise"
    finally:
        fresh.close()
    # an insecure seeded client reproduces its words call by call, and the seeded form leaves the full form's sequence alone
    one, two, three = MyClientKey(0xA11CE), MyClientKey(0xA11CE), MyClientKey(0xA11CE)
    try:
        want = [one.select_query(index, n_chars, row_chars, seeded=True) for _ in range(2)]
        got = [two.select_query(index, n_chars, row_chars, seeded=True) for _ in range(2)]
        for w, g in zip(want, got):
            assert np.array_equal(w.seed, g.seed) and np.array_equal(w.bodies, g.bodies)
        assert not np.array_equal(got[0].seed, got[1].seed) and (got[0].bodies == got[1].bodies).mean() < 0.01
        full_after = one.select_query(index, n_chars, row_chars)[0]          # `one` has made two seeded queries
        full_first = three.select_query(index, n_chars, row_chars)[0]        # `three` none
        assert np.array_equal(full_after, full_first)
        # the noise is not the seed's: the full form of the same call number shares neither masks nor errors with it
        e_full = _row_error(full_first[0, 2], s, index & 1, 0, False)
        e_seeded = _row_error(expand_select_query(want[0])[0, 2], s, index & 1, 0, False)
        assert (e_full == e_seeded).mean() < 0.01
    finally:
        one.close(); two.close(); three.close()


def test_bookkeeping_of_seeded_and_batched_calls_on_a_planner_context(sk):
    from fhestring_amd.api import (FheString, SeededSelectQuery, SELECT_BATCH_MAX_BYTES, SELECT_MAX_BATCH,
                                   SELECT_QUERY_BIT_WORDS, SELECT_SEEDED_BIT_WORDS, select_batch_bytes)
    L, h = sk.ctx._L, sk.ctx._h
    sk.set_mode(1)
    full = np.zeros(SELECT_QUERY_BIT_WORDS, U64)                      # a planner reads no word of a query
    seeded = SeededSelectQuery(np.zeros(8, np.uint32), np.zeros(SELECT_SEEDED_BIT_WORDS, U64), 1)
    x, y, z, w = sk.dummy_string(4).chars
    z.set_noise(9)
    y.set_noise(5)
    a, b = sk.dummy_string(2).chars
    r1, r2 = a.add(sk.trivial(1)), a.add(sk.trivial(2))              # one blind rotation: a rotation group
    sk.flush()
    e = sk.store_put(FheString([x, y, z, w]))
    g = sk.store_put(FheString([r1, b, b, r2]))
    e.rekey()

    def figures(t):
        got = t.get()
        return len(t), t.device_bytes, t.rekeys, [c.sum_c2() for c in got.chars]

    def add_cost(p, q):
        sk.stats(reset=True)
        r = p.add(q)                                                  # (kept alive until the flush)
        sk.flush()
        assert r is not None
        return sk.stats()["max_input_sum_c2"]

    for src in (e, g):
        single = [src.select(full, 2) for _ in range(3)]
        assert [t.id for t in single] == list(range(single[0].id, single[0].id + 3))
        one = src.select(seeded, 2)
        assert one.id == single[-1].id + 1 and figures(one) == figures(single[0])
        for queries in ([full] * 3, [seeded] * 3, [full], [seeded] * SELECT_MAX_BATCH):
            before = sk.store_stats()["entries"]
            many = src.select_many(queries, 2)
            assert [t.id for t in many] == list(range(many[0].id, many[0].id + len(queries)))
            assert sk.store_stats()["entries"] == before + len(queries)
            assert all(figures(t) == figures(single[0]) for t in many)
            for t in many[3:]:
                t.drop()
        assert figures(single[0])[2] == src.rekeys + 2
    # every result of a batch has a rotation group of its own: inside one result the grouped blocks are correlated
    # (tests/test_select.py: 4), across two results of one batch they are strangers (3)
    m1, m2 = (t.get() for t in g.select_many([full, full], 2))
    assert add_cost(m1[0], m1[1]) == 4 and add_cost(m1[0], m2[1]) == 3

    # ---- refused calls create nothing and write 0 to every id
    def batch_rc(eid, row_chars, form, seeds, table, n, bits, ids="own"):
        out = (C.c_uint64 * 80)(*([77] * 80))
        before = sk.store_stats()["entries"]
        rc = L.fhs_store_select_batch(h, eid, row_chars, form, seeds, table, n, bits, None if ids is None else out)
        if rc != 0:
            assert sk.store_stats()["entries"] == before
            assert ids is None or all(out[i] == 0 for i in range(min(n, 64)))
            assert all(out[i] == 77 for i in range(64, 80))
        return rc

    ptrs = lambda arr, n: (C.c_void_p * max(1, n))(*([arr.ctypes.data] * n))
    seeds = np.zeros((80, 8), np.uint32)
    fw, bw = full, seeded.bodies
    assert batch_rc(e.id, 2, 0, None, ptrs(fw, 2), 2, 1) == 0 and batch_rc(e.id, 2, 1, seeds.ctypes.data, ptrs(bw, 2), 2, 1) == 0
    assert batch_rc(12345, 2, 0, None, ptrs(fw, 2), 2, 1) == FHS_ERR_ARG           # unknown id
    assert batch_rc(e.id, 3, 0, None, ptrs(fw, 2), 2, 1) == FHS_ERR_ARG            # a refused shape
    assert batch_rc(e.id, 4, 0, None, ptrs(fw, 2), 2, 1) == FHS_ERR_ARG            # one row
    assert batch_rc(e.id, 2, 0, None, ptrs(fw, 2), 2, 2) == FHS_ERR_ARG            # bits is 1
    assert batch_rc(e.id, 2, 0, None, ptrs(fw, 0), 0, 1) == FHS_ERR_ARG            # n = 0
    assert batch_rc(e.id, 2, 0, None, ptrs(fw, 65), 65, 1) == FHS_ERR_ARG          # n > FHS_SELECT_MAX_BATCH
    assert batch_rc(e.id, 2, 0, None, ptrs(fw, 64), 64, 1) == 0
    assert batch_rc(e.id, 2, 2, None, ptrs(fw, 2), 2, 1) == FHS_ERR_ARG            # no such form
    assert batch_rc(e.id, 2, 0, None, None, 2, 1) == FHS_ERR_ARG                   # null pointers: the table,
    holed = ptrs(fw, 3)
    holed[1] = None
    assert batch_rc(e.id, 2, 0, None, holed, 3, 1) == FHS_ERR_ARG                  # one query,
    assert batch_rc(e.id, 2, 1, None, ptrs(bw, 2), 2, 1) == FHS_ERR_ARG            # the seeds of the seeded form,
    assert batch_rc(e.id, 2, 0, None, ptrs(fw, 2), 2, 1, ids=None) == FHS_ERR_ARG  # the ids
    out = C.c_uint64(77)
    assert L.fhs_store_select_seeded(h, e.id, 2, None, bw.ctypes.data, 1, C.byref(out)) == FHS_ERR_ARG and out.value == 0
    assert L.fhs_store_select_seeded(h, e.id, 2, seeds.ctypes.data, None, 1, C.byref(out)) == FHS_ERR_ARG
    assert L.fhs_store_select_seeded(h, e.id, 2, seeds.ctypes.data, bw.ctypes.data, 2, C.byref(out)) == FHS_ERR_ARG
    assert L.fhs_store_select_seeded(h, e.id, 2, seeds.ctypes.data, bw.ctypes.data, 1, None) == FHS_ERR_ARG
    # the counter limit: 255 re-keys' worth
    for i in range(253 - e.rekeys):
        assert L.fhs_store_rekey(h, e.id, None) == 0
    assert batch_rc(e.id, 2, 0, None, ptrs(fw, 2), 2, 1) == 0
    e.rekey()
    assert batch_rc(e.id, 2, 0, None, ptrs(fw, 2), 2, 1) == FHS_ERR_LIMIT
    assert batch_rc(e.id, 2, 1, seeds.ctypes.data, ptrs(bw, 2), 2, 1) == FHS_ERR_LIMIT
    # the workspace limit: 65536 characters are 128 groups; rows of 64 take 10 bits and 64 queries exactly the limit,
    # rows of 32 take 11 bits
    per_query = lambda bits, groups: bits * 8 * 2 * N * 8 + ((groups + 1) // 2 + (groups + 3) // 4) * 2 * N * 4
    assert select_batch_bytes(65536, 64, 64) == 64 * per_query(10, 128) == SELECT_BATCH_MAX_BYTES == 256 << 20
    assert select_batch_bytes(65536, 32, 64) == 64 * per_query(11, 128) > SELECT_BATCH_MAX_BYTES
    assert select_batch_bytes(2, 1, 1) == per_query(1, 1) == 262144 + 2 * 16384   # (one group: both buffers hold one GLWE)
    assert select_batch_bytes(65536, 64, 0) == 0 and select_batch_bytes(65536, 64, 65) == 0 and select_batch_bytes(6, 4, 1) == 0
    big = sk.store_put(sk.dummy_string(65536))
    q11 = np.zeros(11 * SELECT_QUERY_BIT_WORDS, U64)
    assert batch_rc(big.id, 32, 0, None, ptrs(q11, 64), 64, 11) == FHS_ERR_LIMIT
    assert batch_rc(big.id, 32, 0, None, ptrs(q11, 60), 60, 11) == 0 and batch_rc(big.id, 64, 0, None, ptrs(q11, 64), 64, 10) == 0
    assert big.select(q11, 32).rekeys == 22                            # a single call has no such limit
    # a planner computes nothing: the diagnostic says so
    out = np.zeros((1, 8, 2, N))
    assert L.fhs_debug_select_query_device(h, 0, None, full.ctypes.data, 1, out.ctypes.data) == -3
