"""The GLWE keyswitch family of the string store on the MI355X -- rekey_glwe_kernel, rekey_packed_kernel,
rekey_entry_packed_kernel (rekey_kernels.hip) and select_cmux_kernel with its tree and rotate launches
(select_kernels.hip) -- under synthetic keys and on chosen words, against tests/store_model.py, integer numpy that shares
nothing with the library, and against the host references.  The device half of tests/test_store_synth.py, which lists
the inputs and proves with negative controls that they tell a right kernel from a subtly wrong one.

The smoke run compares device and host under a real client key, where a tie or a wrap of the stored word after the
keyswitch sum appears with probability 2^-32 per word, and host and device share storage_words.h and their formulas.
Here the model's input is what was uploaded, never a download:

    identity key      the re-key returns its input: raw words, imported entries in place and as a copy, the recipient's
                      packed download against the own-key one at every window, rekey_packed against its closed form
    monomial keys     every key of test_store_synth.py in all three formats, and an entry re-keyed in place
    gadget queries    the select returns the source row's own words (or zeros for a missing node): raw, by entry, in batches
    monomial queries  both queries of test_store_synth.py at its four shapes
    dense, extreme    extreme and off-grid words in every coefficient, and every digit -2^15 under the largest key word

One context in exact arithmetic for the module, no bootstrap anywhere; every test loads its own re-key key and unloads it.
No tolerance anywhere.  Like tests/test_pack_synth_device.py this file carries no `gpu` mark: every test skips unless a
device is visible, and none is touched while the file is collected.  Figures are printed per case (pytest -s)."""
import time

import numpy as np
import pytest

import store_model as sm

N = 2048
U64 = np.uint64


@pytest.fixture(scope="module")
def sk(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from fhestring_amd.api import MyServerKey
    keys = request.getfixturevalue("oracle_keys")
    s = MyServerKey.from_raw_keys(keys.bsk, keys.ksk, arith=0)
    yield s
    s.close()


def _same(got, want, what):
    for g, w, name in zip(got, want, ("mask", "body")):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what)
        assert np.array_equal(g, w), "%s: %s, %d words differ" % (name, what, int((g != w).sum()))


def _raw(p):
    return p if isinstance(p, tuple) else (p.mask16, p.body16)


def _words(c):
    return c.mask32, c.body32


def _compact(n_chars):
    from fhestring_amd.api import CompactFheString
    return CompactFheString(n_chars, *sm.entry_words(n_chars))


# ---- re-key ------------------------------------------------------------------------------------------------------------
def test_identity_key_returns_its_input(sk):
    sk.load_rekey_key(sm.rekey_key(sm.identity_key()))
    try:
        for n_blocks in sm.BLOCK_COUNTS:
            mask, body = sm.rekey_words(n_blocks)
            _same(sk.ctx.rekey_device(mask, body, n_blocks), (mask, body), ("identity", n_blocks))
            m64, b64 = sm.packed_words(n_blocks)
            want = sm.round16(sm.round32(m64).astype(U64) << U64(32)), sm.round16(b64).reshape(-1)[:n_blocks]
            _same(sk.ctx.rekey_packed_device(m64, b64, n_blocks), want, ("identity, packed", n_blocks))
        for n_chars in sm.WINDOW_CHARS:
            c = _compact(n_chars)
            e = sk.store_import(c)
            try:
                for first, count in sm.windows(n_chars):
                    own, other = e.download_packed(first, count), e.download_packed(first, count, recipient=True)
                    assert own.first_coef == other.first_coef
                    _same(_raw(other), _raw(own), ("identity against the own-key switch", n_chars, first, count))
                    _same(_raw(own), sm.store_packed(None, c.mask32, c.body32, 4 * n_chars, first, count)[:2], ("own key", n_chars, first, count))
                f = e.rekey(copy=True)
                try:
                    _same(_words(f.export()[0]), _words(c), ("identity, as a copy", n_chars))
                finally:
                    f.drop()
                assert e.rekey() is e
                _same(_words(e.export()[0]), _words(c), ("identity, in place", n_chars))
            finally:
                e.drop()
    finally:
        sk.load_rekey_key(None)


def test_monomial_keys_equal_the_model_and_the_host(sk):
    from fhestring_amd.api import rekey_host, rekey_packed_host, store_packed_host
    total = sm.Tally()
    for name, spec in sm.rekey_specs().items():
        key = sm.rekey_key(spec)
        sk.load_rekey_key(key)
        try:
            t0, host = time.perf_counter(), 0.0
            for n_blocks in sm.BLOCK_COUNTS:
                mask, body = sm.rekey_words(n_blocks)
                want = sm.rekey(spec, mask, body, n_blocks, tally=total)
                t1 = time.perf_counter()
                _same(rekey_host(key, mask, body, n_blocks), want, ("host, re-key", name, n_blocks))
                host += time.perf_counter() - t1
                _same(sk.ctx.rekey_device(mask, body, n_blocks), want, ("re-key", name, n_blocks))
                m64, b64 = sm.packed_words(n_blocks)
                want = sm.rekey_packed(spec, m64, b64, n_blocks, tally=total)
                t1 = time.perf_counter()
                _same(_raw(rekey_packed_host(key, m64, b64, n_blocks)), want, ("host, packed", name, n_blocks))
                host += time.perf_counter() - t1
                _same(sk.ctx.rekey_packed_device(m64, b64, n_blocks), want, ("packed", name, n_blocks))
            for n_chars in sm.WINDOW_CHARS:
                c = _compact(n_chars)
                e = sk.store_import(c)
                try:
                    for first, count in sm.windows(n_chars):
                        want = sm.store_packed(spec, c.mask32, c.body32, 4 * n_chars, first, count, tally=total)
                        t1 = time.perf_counter()
                        _same(_raw(store_packed_host(key, c, first, count)), want[:2], ("host, window", name, n_chars, first, count))
                        host += time.perf_counter() - t1
                        got = e.download_packed(first, count, recipient=True)
                        assert got.first_coef == want[2]
                        _same(_raw(got), want[:2], ("window", name, n_chars, first, count))
                    _same(_words(e.export()[0]), _words(c), ("the entry after its downloads", name, n_chars))
                    # in place: every key here shifts the mask, so a store ahead of the kernel's barrier would show
                    assert e.rekey() is e and e.rekeys == 1
                    _same(_words(e.export()[0]), sm.rekey(spec, c.mask32, c.body32, 4 * n_chars), ("in place", name, n_chars))
                finally:
                    e.drop()
            print("key with %s: %.3f s, of which the host references %.3f s" % (name, time.perf_counter() - t0, host))
        finally:
            sk.load_rekey_key(None)
    print("boundaries reached under the monomial re-key keys:\n%s" % total)
    assert all(hits > 0 for hits in total.counts.values()), total.counts


# ---- select ------------------------------------------------------------------------------------------------------------
def _gadget_indices(n_chars, row_chars):
    """0, R - 1, both sides of a group boundary, and one missing node where there is one"""
    groups, _, rot, levels = sm.geometry(n_chars, row_chars)
    rows, per_group = n_chars // row_chars, 1 << rot
    idx = {0, rows - 1, min(per_group, rows) - 1, min(per_group, rows - 1)}
    if groups < 1 << levels:
        idx.add(groups << rot)
    assert all(sm.names_a_row_or_a_missing_node(n_chars, row_chars, i) for i in idx)
    return sorted(idx)


def test_gadget_queries_return_the_source_row(sk):
    from fhestring_amd.api import CompactFheString
    for n_chars, row_chars in sm.SHAPES:
        _, _, rot, levels = sm.geometry(n_chars, row_chars)
        bits = rot + levels
        mask, body = sm.entry_words(n_chars)
        idx = _gadget_indices(n_chars, row_chars)
        queries = [sm.query(sm.gadget_query(i, bits)) for i in idx]
        want = [sm.selected_row(mask, body, n_chars, row_chars, i) for i in idx]
        t0 = time.perf_counter()
        e = sk.store_import(CompactFheString(n_chars, mask, body))
        try:
            for i, q, w in zip(idx, queries, want):
                _same(sk.ctx.select_device(q, mask, body, 4 * n_chars, row_chars), w, ("raw", n_chars, row_chars, i))
                f = e.select(q, row_chars)
                try:
                    assert len(f) == row_chars
                    _same(_words(f.export()[0]), w, ("entry", n_chars, row_chars, i))
                finally:
                    f.drop()
            last = len(idx) - 1
            for pick in ((last,), (0, last), (0, 1, last, 1, 0)):           # batches of 1, 2 and 5, queries twice in the last
                out = e.select_many([queries[k] for k in pick], row_chars)
                try:
                    for f, k in zip(out, pick):
                        _same(_words(f.export()[0]), want[k], ("batch", n_chars, row_chars, pick, idx[k]))
                finally:
                    for f in out:
                        f.drop()
            got = e.export()[0]
            _same(_words(got), (mask, body), ("the source entry", n_chars, row_chars))
        finally:
            e.drop()
        print("gadget queries, %d x %d characters, indices %s: %.3f s" % (n_chars // row_chars, row_chars, idx, time.perf_counter() - t0))


def test_monomial_queries_equal_the_model_and_the_host(sk):
    from fhestring_amd.api import CompactFheString, select_host
    total = sm.Tally()
    for n_chars, row_chars in sm.MONOMIAL_SHAPES:
        _, _, rot, levels = sm.geometry(n_chars, row_chars)
        mask, body = sm.entry_words(n_chars)
        e = sk.store_import(CompactFheString(n_chars, mask, body))
        try:
            for name, spec in sm.select_specs(rot + levels).items():
                q = sm.query(spec)
                want = sm.select(spec, mask, body, n_chars, row_chars, tally=total)
                _same(select_host(q, mask, body, 4 * n_chars, row_chars), want, ("host", name, n_chars, row_chars))
                _same(sk.ctx.select_device(q, mask, body, 4 * n_chars, row_chars), want, ("raw", name, n_chars, row_chars))
                f = e.select(q, row_chars)
                try:
                    _same(_words(f.export()[0]), want, ("entry", name, n_chars, row_chars))
                finally:
                    f.drop()
            _same(_words(e.export()[0]), (mask, body), ("the source entry", n_chars, row_chars))
        finally:
            e.drop()
    print("boundaries reached under the monomial queries:\n%s" % total)
    assert all(hits > 0 for hits in total.counts.values()), total.counts


# ---- dense keys and the top of the exact range -------------------------------------------------------------------------------
def _dense_rekey(sk, key, n_blocks, mask, body, m64, b64, what):
    from fhestring_amd.api import CompactFheString, rekey_host, rekey_packed_host, store_packed_host
    sk.load_rekey_key(key)
    try:
        _same(sk.ctx.rekey_device(mask, body, n_blocks), rekey_host(key, mask, body, n_blocks), (what, "re-key"))
        _same(sk.ctx.rekey_packed_device(m64, b64, n_blocks), _raw(rekey_packed_host(key, m64, b64, n_blocks)), (what, "packed"))
        n_chars = n_blocks // 4
        c = CompactFheString(n_chars, mask, body)
        e = sk.store_import(c)
        try:
            for first, count in ((0, n_chars), (n_chars // 2, n_chars - n_chars // 2)):
                _same(_raw(e.download_packed(first, count, recipient=True)), _raw(store_packed_host(key, c, first, count)),
                      (what, "window", first, count))
        finally:
            e.drop()
    finally:
        sk.load_rekey_key(None)


def test_dense_extreme_keys_equal_the_host(sk):
    from fhestring_amd.api import REKEY_KEY_WORDS, SELECT_QUERY_BIT_WORDS, select_host
    rng = np.random.default_rng(5)                           # (the key and the queries of the CPU file's test)
    key = rng.choice(np.array(sm.pm.KEY_WORDS, U64), REKEY_KEY_WORDS)
    n_blocks = 2052
    _dense_rekey(sk, key, n_blocks, *sm.rekey_words(n_blocks), *sm.packed_words(n_blocks), "dense key")
    for n_chars, row_chars in ((2, 1), (1536, 512)):
        _, _, rot, levels = sm.geometry(n_chars, row_chars)
        query = rng.choice(np.array(sm.pm.KEY_WORDS, U64), (rot + levels) * SELECT_QUERY_BIT_WORDS).reshape(-1, 4, 2, N)
        m, b = sm.entry_words(n_chars)
        _same(sk.ctx.select_device(query, m, b, 4 * n_chars, row_chars), select_host(query, m, b, 4 * n_chars, row_chars),
              ("dense query", n_chars, row_chars))


def test_every_digit_minus_2_15_under_the_largest_key(sk):
    """the largest true sums the two instantiations can meet, 2^84 and 2^85 grid units (tests/test_store_synth.py holds
    the host references against the schoolbook product on these inputs, and the figures)"""
    from fhestring_amd.api import REKEY_KEY_WORDS, SELECT_QUERY_BIT_WORDS, select_host
    n_blocks = N
    key = np.full(REKEY_KEY_WORDS, sm.EXTREME_KEY_WORD, U64)
    mask, body = np.full((1, N), sm.EXTREME_WORD, np.uint32), np.full(n_blocks, sm.EXTREME_WORD, np.uint32)
    m64, b64 = sm.packed_words(n_blocks)
    m64[:] = U64(sm.EXTREME_WORD) << U64(32)
    _dense_rekey(sk, key, n_blocks, mask, body, m64, b64, "all -2^15")
    n_chars, row_chars = 1024, 512                           # one tree level, no rotate: a = group 0 = 0, b = group 1
    query = np.full(SELECT_QUERY_BIT_WORDS, sm.EXTREME_KEY_WORD, U64).reshape(1, 4, 2, N)
    m, b = np.zeros((2, N), np.uint32), np.zeros(2 * N, np.uint32)
    m[1], b[N:] = sm.EXTREME_WORD, sm.EXTREME_WORD
    want = select_host(query, m, b, 4 * n_chars, row_chars)
    _same(sk.ctx.select_device(query, m, b, 4 * n_chars, row_chars), want, ("all -2^15", "select"))
    _same(want, sm.select(query, m, b, n_chars, row_chars), ("all -2^15", "select, host against the schoolbook"))
