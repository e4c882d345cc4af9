"""The packing tree's kernels (pack_kernels.hip: pack_level_kernel<LEAF>, pack_switch16_kernel; the store's 32-bit
switch) on the MI355X under synthetic packing keys and on chosen words, against tests/pack_model.py -- integer numpy
that shares nothing with the library -- and against fhs_pack_host.  The device half of tests/test_pack_synth.py, which
lists the inputs and proves with negative controls that they tell a right tree from a subtly wrong one.

tests/test_gpu_packed.py and tests/test_gpu_store.py compare device and host on real ciphertexts under a real key, where
a wrong index, sign or rounding shows only by chance, and host and device share their formulas.  Here the inputs are
strings of arbitrary words (the tree does not care whether a row is a ciphertext), some characters trivial, and the
model's input is what was uploaded, never a download:

    zero key        1 .. 2049 characters against the closed form; 2049 characters are five groups in two passes, the
                    first check of the second pass's offsets that does not rest on the device
    monomial keys   both keys of test_pack_synth.py against the recursion and the host reference
    dense key       extreme and off-grid words in every key coefficient, against the host reference
    store           store_put / export / get under a monomial key: round32 of the model, and its sample extraction
                    (the boundary words of the 32-bit rounding itself are test_store.py's, on the host)
    off-grid keys   the re-key and the select under random keys that do not lie on the 2^6 grid, against their references

One context in exact arithmetic for the module, no bootstrap anywhere; fhs_load_packing_key on a live context replaces
the key, so every test loads its own.  No tolerance anywhere.  Like tests/test_sched_parity_device.py this file carries
no `gpu` mark: every test skips unless a device is visible, and none is touched while the file is collected.  Figures
are printed per case (pytest -s)."""
import time

import numpy as np
import pytest

import pack_model as pm
from ring_util import round16, round32

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


def _string(sk, seed, n_chars):
    """-> (the characters on the device, the blocks [4 n][2049] the model packs): arbitrary words, six in ten of them
    chosen; every seventh block with an all-zero mask; every fifth character (from the second) a trivial one"""
    rng = np.random.default_rng(seed)
    blocks = pm.chosen_blocks(rng, 4 * n_chars, [k for k in range(4 * n_chars) if k % 7 == 3]).reshape(n_chars, 4, pm.BIG_CT)
    blocks[::2, :, N] = rng.choice(np.array(pm.ROUND16_BODY_WORDS, U64), blocks[::2, :, N].shape)
    chars = sk.upload_string(blocks).chars
    for i in range(1, n_chars, 5):
        v = int(rng.integers(0, 256))
        chars[i] = sk.trivial(v)
        blocks[i] = pm.trivial_char(v)
    return chars, blocks.reshape(-1, pm.BIG_CT)


def _same(got, want, what):
    m64, b64 = got
    assert np.array_equal(m64, want[0]), "mask64: %s" % (what,)
    assert np.array_equal(b64, want[1]), "body64: %s" % (what,)


def _download(sk, chars, want, what):
    """the wide download equals `want` in its 64-bit words, round16 of it in its 16-bit words, and the plain download
    has the same bytes"""
    n_blocks = 4 * len(chars)
    t0 = time.perf_counter()
    p, m64, b64 = sk.download_packed(chars, wide=True)
    dt = time.perf_counter() - t0
    _same((m64, b64), want, what)
    assert np.array_equal(p.mask16, round16(want[0])), "mask16: %s" % (what,)
    assert np.array_equal(p.body16, round16(want[1]).reshape(-1)[:n_blocks]), "body16: %s" % (what,)
    assert sk.download_packed(chars).to_bytes() == p.to_bytes(), "plain download: %s" % (what,)
    return dt


def test_zero_key_equals_the_closed_form(sk):
    from fhestring_amd.api import PACK_KEY_WORDS
    sk.load_packing_key(np.zeros(PACK_KEY_WORDS, U64))
    tally = pm.Tally()
    for n_chars in (1, 3, 6, 75, 512, 513, 2049):
        chars, blocks = _string(sk, n_chars, n_chars)
        want = pm.zero_key_pack(blocks)
        dt = _download(sk, chars, want, ("zero key", n_chars))
        live = want[1].reshape(-1)[:4 * n_chars]
        tally.prescale_words(blocks)
        tally.add(pm.round_classes(want[0], 48))
        tally.add(pm.round_classes(live, 48))
        print("zero key, %d characters: device %.3f s" % (n_chars, dt))
        del chars
    print("boundaries reached under the zero key:\n%s" % tally)
    assert all(hits > 0 for hits in tally.counts.values()), tally.counts


def test_monomial_keys_equal_the_recursion_and_the_host(sk):
    from fhestring_amd.api import pack_host
    for name, spec in pm.monomial_specs().items():
        key = pm.monomial_key(spec)
        sk.load_packing_key(key)
        tally = pm.Tally()
        for n_chars in (1, 3, 6, 75, 513):
            chars, blocks = _string(sk, 100 + n_chars, n_chars)
            want = pm.tree(spec, blocks, tally=tally)
            _same(pack_host(key, blocks), want, ("host", name, n_chars))
            dt = _download(sk, chars, want, (name, n_chars))
            print("key with %s, %d characters: device %.3f s" % (name, n_chars, dt))
            del chars
        print("boundaries reached under the key with %s:\n%s" % (name, tally))
        assert all(hits > 0 for hits in tally.counts.values()), tally.counts


def test_dense_extreme_key_equals_the_host(sk):
    from fhestring_amd.api import PACK_KEY_WORDS, pack_host
    key = np.random.default_rng(3).choice(np.array(pm.KEY_WORDS, U64), PACK_KEY_WORDS)
    sk.load_packing_key(key)
    for n_chars in (6, 75):
        chars, blocks = _string(sk, 200 + n_chars, n_chars)
        dt = _download(sk, chars, pack_host(key, blocks), ("dense key", n_chars))
        print("dense key, %d characters: device %.3f s" % (n_chars, dt))
        del chars


def test_store_put_export_and_get_under_a_monomial_key(sk):
    from fhestring_amd.api import CompactFheString
    from test_public_key import _numpy_expand
    spec = pm.monomial_specs()["scattered exponents"]
    sk.load_packing_key(pm.monomial_key(spec))
    for n_chars in (6, 513):
        chars, blocks = _string(sk, 300 + n_chars, n_chars)
        m64, b64 = pm.tree(spec, blocks)
        want = CompactFheString(n_chars, round32(m64), round32(b64).reshape(-1)[:4 * n_chars])
        t0 = time.perf_counter()
        e = sk.store_put(chars)
        got = e.export()[0]
        assert np.array_equal(got.mask32, want.mask32), ("mask32", n_chars)
        assert np.array_equal(got.body32, want.body32), ("body32", n_chars)
        back = e.get().download()
        dt = time.perf_counter() - t0
        assert np.array_equal(back, _numpy_expand(want, 0, n_chars)), ("get", n_chars)
        print("store under a monomial key, %d characters: put, export, get and download %.3f s" % (n_chars, dt))
        e.drop()
        del chars


def test_rekey_and_select_under_keys_off_the_grid(sk):
    """on the device these two have only been loaded with keys on the grid; the references round a key first"""
    from fhestring_amd.api import REKEY_KEY_WORDS, SELECT_QUERY_BIT_WORDS, rekey_host, select_bits, select_host
    rng = np.random.default_rng(41)
    key = rng.integers(0, 1 << 64, REKEY_KEY_WORDS, dtype=U64)
    assert (key & U64(63)).any()
    sk.load_rekey_key(key)
    try:
        n_blocks = 2052
        mask = rng.integers(0, 1 << 32, (2, N), dtype=np.uint32)
        body = rng.integers(0, 1 << 32, n_blocks, dtype=np.uint32)
        got, want = sk.ctx.rekey_device(mask, body, n_blocks), rekey_host(key, mask, body, n_blocks)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "re-key under an off-grid key"
    finally:
        sk.load_rekey_key(None)
    n_chars, row_chars = 1536, 512
    bits = select_bits(n_chars, row_chars)
    assert bits > 0
    query = rng.integers(0, 1 << 64, bits * SELECT_QUERY_BIT_WORDS, dtype=U64)
    assert (query & U64(63)).any()
    mask = rng.integers(0, 1 << 32, (3, N), dtype=np.uint32)
    body = rng.integers(0, 1 << 32, 4 * n_chars, dtype=np.uint32)
    got = sk.ctx.select_device(query, mask, body, 4 * n_chars, row_chars)
    want = select_host(query, mask, body, 4 * n_chars, row_chars)
    assert np.array_equal(got[0].reshape(-1), want[0].reshape(-1)) and np.array_equal(got[1], want[1]), \
        "select under an off-grid query"
