"""Key load on the MI355X: keys that do not lie on the key grid in all six blind-rotation kernels, and key replacement
on a live context.  The device half of tests/test_key_load.py, which anchors the integer references to the oracle and
shows with negative controls that the rows tell a right rounding from a wrong one.

    off-grid keys   tests/synth_key.py: offgrid_material().  bsk_to_fft_kernel rounds every word to 2^6 on the device for
                    the classic Fourier key and the f64 pair key, convert_bsk_to_ntt rounds on the host, to 2^6 for the
                    classic key and -- from the original word -- to 2^7 for the exact pair key.  The exact kernels equal
                    the integer references in every word, the f64 kernels their mirrors (oracle modes 3 and 4) bit for
                    bit, and stay within T3 / T4 (words that return to the grid, words that move by a grid step) and
                    T3U / T4U (uniformly random words) of the integer references on one-product rows.  The rows that meet
                    only words that return give what the same context gives under the on-grid key.
    replacement     keys A and B from different seeds on ONE context, in every order of loading and selecting that
                    decides which derived key is built when: a stale Fourier key, pair key or auxiliary key shows as
                    key A's outputs, or as a call that should fail and does not.
    compressed      a client's seeded key over a plain one and a plain one over it.

Like tests/test_pack_synth_device.py this file carries no `gpu` mark: every test skips unless a device is visible, and
none is touched while the file is collected.  The mirrors are built once per distinct row and module."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import synth_key as sk

# The library's default of fhs_set_fft4_max_batch, restated as in tests/test_gpu_synth_key.py (the C ABI has a setter only)
FFT4_MAX_BATCH_DEFAULT = 512
U = np.uint64


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")


def _no_ksk():
    from oracle import core
    return np.zeros(core.KSK_WORDS, U)                 # the blind-rotation entry never keyswitches


def _mirror(osk, ms, luts, lut_idx, mode, rows=None):
    """Extracted outputs of an oracle mode -> {row: [2049]}, a few rows at a time (ctypes releases the GIL)."""
    rows = list(range(len(ms))) if rows is None else list(rows)
    with ThreadPoolExecutor(4) as pool:
        outs = pool.map(lambda r: sk.sample_extract(osk.blind_rotate(ms[r], luts[lut_idx[r]], mode=mode).reshape(2, sk.N)), rows)
        return dict(zip(rows, outs))


def _run(ctx, arith, ks, lut_idx, luts, n=None, fft4_max=None):
    """blind_rotate_batch in the given arithmetic on the rows tiled to n -> (outputs, the row each one repeats)."""
    src = np.arange(n or len(ks)) % len(ks)
    ctx.set_arithmetic(arith)
    if fft4_max is not None:
        ctx.set_fft4_max_batch(fft4_max)              # 0: the 2-wavefront kernel; 1 << 30: the 4-wavefront ones
    try:
        return ctx.blind_rotate_batch(ks[src], lut_idx[src], luts), src
    finally:
        ctx.set_fft4_max_batch(FFT4_MAX_BATCH_DEFAULT)
        ctx.set_arithmetic(ctx.ARITH_EXACT_NTT)


def _bad(got, src, want):
    return [(b, int(src[b])) for b in range(len(got)) if not np.array_equal(got[b], want[src[b]])]


def _load_everything(c, bsk, bsk_mb2):
    """The key and the pair key in both of their forms, as tests/test_gpu_synth_key.py's fixture does; leaves the exact
    arithmetic selected."""
    c.set_arithmetic(c.ARITH_F64_FFT)                 # builds the Fourier-domain key beside the residues
    c.load_server_key(bsk, _no_ksk())
    c.load_multibit_key(bsk_mb2)
    c.set_arithmetic(c.ARITH_EXACT_NTT)
    c.load_multibit_key(bsk_mb2)


# ---- a. keys off the grid --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mat(gpu):
    return sk.offgrid_material()


@pytest.fixture(scope="module")
def ref(gpu):
    return sk.offgrid_references()


@pytest.fixture(scope="module")
def ctx(mat):
    import fhestring_amd
    c = fhestring_amd.Context(0)
    _load_everything(c, mat.bsk, mat.bsk_mb2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mirrors(mat):
    """{3: [R][2049], 4: [R][2049]}: the oracle rounds the loaded words in its own code."""
    from oracle import core
    osk = core.ServerKey(mat.bsk, _no_ksk()).set_mb2(mat.bsk_mb2)
    out = {}
    for mode in (3, 4):
        by_row = _mirror(osk, mat.ms, mat.luts, mat.lut_idx, mode)
        out[mode] = np.stack([by_row[r] for r in range(len(mat.ms))])
    return out


def _one_product_rows(mat, pair_key):
    """-> (rows of class R and M with one product, rows whose last step is their one product with class U)"""
    kinds = ("single", "pair") if pair_key else ("single",)
    r_rows, one_m, one_u = (mat.r_rows_mb2, mat.one_m_mb2, mat.one_u_mb2) if pair_key else (mat.r_rows, mat.one_m, mat.one_u)
    return [r for r in r_rows if mat.kinds[r] in kinds] + one_m, one_u


def test_exact_kernels_equal_the_integer_references_under_the_off_grid_key(ctx, mat, ref):
    for n in (None, 300):
        got, src = _run(ctx, ctx.ARITH_EXACT_NTT, mat.ks, mat.lut_idx, mat.luts, n)
        assert _bad(got, src, ref.out) == [], ("exact, 2^6 grid", n)
        got, src = _run(ctx, ctx.ARITH_EXACT_NTT_MB2, mat.ks, mat.lut_idx, mat.luts, n)
        assert _bad(got, src, ref.out_mb2_7) == [], ("exact two-bit, 2^7 grid", n)


def test_f64_fft_kernels_equal_their_mirror_under_the_off_grid_key(ctx, mat, ref, mirrors):
    one, one_u = _one_product_rows(mat, False)
    assert len(one) >= 18 and len(one_u) >= 9
    # the routes as in tests/test_gpu_synth_key.py: B * 4 <= slots -> the wide-LDS variant, more -> the shared-area one
    ctx.set_arithmetic(ctx.ARITH_F64_FFT)
    slots = ctx._L.fhs_resident_slots(ctx._h)
    ctx.set_arithmetic(ctx.ARITH_EXACT_NTT)
    assert 4 * len(mat.ks) <= slots, "the row set no longer fits the wide-LDS variant of the 4-wavefront kernel"
    for fft4_max, n in ((0, None), (1 << 30, None), (1 << 30, max(300, slots // 4 + 1))):
        got, src = _run(ctx, ctx.ARITH_F64_FFT, mat.ks, mat.lut_idx, mat.luts, n, fft4_max)
        assert _bad(got, src, mirrors[3]) == [], (fft4_max, n)
        worst = max(sk.centred_abs_max(got[r], ref.out[r]) for r in one)
        worst_u = max(sk.centred_abs_max(got[r], ref.out[r]) for r in one_u)
        assert worst < sk.T3 and worst_u < sk.T3U, (fft4_max, n, worst, worst_u)


def test_f64_two_bit_kernel_equals_its_mirror_under_the_off_grid_key(ctx, mat, ref, mirrors):
    one, one_u = _one_product_rows(mat, True)
    assert len(one) >= 26 and len(one_u) >= 13
    for n in (None, 300):
        got, src = _run(ctx, ctx.ARITH_F64_FFT_MB2, mat.ks, mat.lut_idx, mat.luts, n)
        assert _bad(got, src, mirrors[4]) == [], n
        worst = max(sk.centred_abs_max(got[r], ref.out_mb2_6[r]) for r in one)
        worst_u = max(sk.centred_abs_max(got[r], ref.out_mb2_6[r]) for r in one_u)
        assert worst < sk.T4 and worst_u < sk.T4U, (n, worst, worst_u)


def test_rows_that_meet_only_returning_words_equal_the_on_grid_key_on_the_same_context(ctx, mat):
    """Every arithmetic and f64 route on the rows of class R, under the off-grid key and then under material()'s key
    loaded into the same context: word for word the same.  (Runs last of the off-grid items and puts their key back.)"""
    base = sk.material()
    runs = [(ctx.ARITH_EXACT_NTT, None, mat.r_rows), (ctx.ARITH_F64_FFT, 0, mat.r_rows), (ctx.ARITH_F64_FFT, 1 << 30, mat.r_rows),
            (ctx.ARITH_EXACT_NTT_MB2, None, mat.r_rows_mb2), (ctx.ARITH_F64_FFT_MB2, None, mat.r_rows_mb2)]
    def outputs():
        return [_run(ctx, arith, mat.ks[rows], mat.lut_idx[rows], mat.luts, None, fft4_max)[0] for arith, fft4_max, rows in runs]
    assert len(mat.r_rows) >= 40 and len(mat.r_rows_mb2) >= 40
    off_grid = outputs()
    try:
        _load_everything(ctx, base.bsk, base.bsk_mb2)
        on_grid = outputs()
    finally:
        _load_everything(ctx, mat.bsk, mat.bsk_mb2)
    for (arith, fft4_max, rows), a, b in zip(runs, off_grid, on_grid):
        assert [rows[k] for k in range(len(rows)) if not np.array_equal(a[k], b[k])] == [], (arith, fft4_max)
    want = sk.references()
    assert np.array_equal(on_grid[0], want.out[mat.r_rows]) and np.array_equal(on_grid[3], want.out_mb2[mat.r_rows_mb2])


# ---- b. key replacement ----------------------------------------------------------------------------------------------

class _Key:
    pass


def _rows():
    """The rows of items b and c: material()'s one-product and two-product rows, six sparse ones and a full one."""
    m = sk.material()
    return sk.rows_of(m, "single", "pair") + sk.rows_of(m, "sparse")[:6] + sk.rows_of(m, "full")[:1]


@functools.lru_cache(maxsize=None)
def _keys():
    """A: material()'s keys.  B: monomial keys of other key bits from another seed.  Each with the integer references and
    the mirrors on _rows() -> out, out_mb2, m3, m4 [rows][2049]."""
    from oracle import core
    m, rows = sk.material(), _rows()
    a, b = _Key(), _Key()
    a.bsk, a.bsk_mb2 = m.bsk, m.bsk_mb2
    a.out, a.out_mb2 = sk.references().out[rows], sk.references().out_mb2[rows]
    rng = np.random.default_rng(0xB0B)
    s = rng.integers(0, 2, sk.LWE_N).astype(np.int64)
    b.bsk, desc = sk.monomial_key(sk.LWE_N, s, rng)
    b.bsk_mb2, desc_mb2 = sk.monomial_key(3 * (sk.LWE_N // 2), sk.pair_bits(s), rng)
    b.out = np.stack([sk.sample_extract(sk.blind_rotate_ref(desc, m.ms[r], m.luts[m.lut_idx[r]])) for r in rows])
    b.out_mb2 = np.stack([sk.sample_extract(sk.blind_rotate_mb2_ref(desc_mb2, m.ms[r], m.luts[m.lut_idx[r]])) for r in rows])
    for k in (a, b):
        osk = core.ServerKey(k.bsk, _no_ksk()).set_mb2(k.bsk_mb2)
        for mode, name in ((3, "m3"), (4, "m4")):
            by_row = _mirror(osk, m.ms, m.luts, m.lut_idx, mode, rows)
            setattr(k, name, np.stack([by_row[r] for r in rows]))
    return a, b


@pytest.fixture(scope="module")
def keys(gpu):
    return _keys()


@pytest.fixture(scope="module")
def live(gpu):
    """The one context of items b and c."""
    import fhestring_amd
    c = fhestring_amd.Context(0)
    yield c
    c.close()


def _check(c, arith, want, what, differs_from=None):
    """The rows of items b and c in one arithmetic (the f64 FFT one on both routes) equal `want` in every word, and, where
    given, differ from `differs_from` on every row."""
    m, rows = sk.material(), _rows()
    for fft4_max in ((0, 1 << 30) if arith == c.ARITH_F64_FFT else (None,)):
        got, src = _run(c, arith, m.ks[rows], m.lut_idx[rows], m.luts, None, fft4_max)
        assert _bad(got, src, want) == [], (what, fft4_max)
        if differs_from is not None:
            assert [k for k in range(len(rows)) if np.array_equal(got[k], differs_from[k])] == [], (what, fft4_max)


def _refused(c, call, needle):
    """`call` raises FhsError with code -3 and a message that names what is missing."""
    import fhestring_amd
    with pytest.raises(fhestring_amd.FhsError) as e:
        call()
    assert e.value.code == -3 and needle in str(e.value), str(e.value)


def test_the_rows_tell_key_a_from_key_b(keys):
    a, b = keys
    for name in ("out", "out_mb2", "m3", "m4"):
        same = [k for k in range(len(_rows())) if np.array_equal(getattr(a, name)[k], getattr(b, name)[k])]
        assert same == [], name
    assert len(_rows()) == 33


def test_a_new_server_key_replaces_every_key_derived_from_the_old_one(live, keys):
    from fhestring_amd.api import PACK_KEY_WORDS, REKEY_KEY_WORDS, CompactFheString, MyServerKey
    c, (a, b) = live, keys
    EXACT, F64, F64_MB2, EXACT_MB2 = c.ARITH_EXACT_NTT, c.ARITH_F64_FFT, c.ARITH_F64_FFT_MB2, c.ARITH_EXACT_NTT_MB2
    # 1. key A under the exact arithmetic, with its pair key
    c.set_arithmetic(EXACT)
    c.load_server_key(a.bsk, _no_ksk())
    c.load_multibit_key(a.bsk_mb2)
    _check(c, EXACT, a.out, "1: exact, A")
    _check(c, EXACT_MB2, a.out_mb2, "1: exact two-bit, A")
    # 2. the f64 arithmetic selected afterwards builds the Fourier key now; the f64 pair key beside it
    c.set_arithmetic(F64)
    c.load_multibit_key(a.bsk_mb2)
    _check(c, F64, a.m3, "2: f64, A")
    _check(c, F64_MB2, a.m4, "2: f64 two-bit, A")
    # 3. key B under the exact arithmetic: the Fourier key and both pair keys of A go
    c.set_arithmetic(EXACT)
    c.load_server_key(b.bsk, _no_ksk())
    _check(c, EXACT, b.out, "3: exact, B", a.out)
    # 4. the Fourier key is built again, from B
    _check(c, F64, b.m3, "4: f64, B", a.m3)
    # 5. no pair key: neither two-bit arithmetic can be selected, and the selected one stays
    for arith in (F64_MB2, EXACT_MB2):
        _refused(c, lambda: c.set_arithmetic(arith), "pair key")
        assert c.arithmetic == EXACT
    # 6. B's pair key in each arithmetic
    c.load_multibit_key(b.bsk_mb2)
    _check(c, EXACT_MB2, b.out_mb2, "6: exact two-bit, B", a.out_mb2)
    _refused(c, lambda: c.set_arithmetic(F64_MB2), "pair key")
    c.set_arithmetic(F64)
    c.load_multibit_key(b.bsk_mb2)
    _check(c, F64_MB2, b.m4, "6: f64 two-bit, B", a.m4)
    _check(c, EXACT_MB2, b.out_mb2, "6: exact two-bit, B, again")
    # 7. key A while the f64 arithmetic is selected: converted at once
    c.set_arithmetic(F64)
    c.load_server_key(a.bsk, _no_ksk())
    assert c.arithmetic == F64
    _check(c, F64, a.m3, "7: f64, A", b.m3)
    _check(c, EXACT, a.out, "7: exact, A", b.out)
    for arith in (F64_MB2, EXACT_MB2):
        _refused(c, lambda: c.set_arithmetic(arith), "pair key")
    # 8. a packing key and a re-key key go with the server key they were loaded under
    s = MyServerKey(c)
    words = np.random.default_rng(8).integers(0, 1 << 64, (2, 4, sk.N + 1), dtype=U)
    entry = s.store_import(CompactFheString(2, np.zeros((1, sk.N), np.uint32), np.arange(8, dtype=np.uint32)))
    s.load_packing_key(np.zeros(PACK_KEY_WORDS, U))
    s.load_rekey_key(np.zeros(REKEY_KEY_WORDS, U))
    assert len(s.download_packed(s.upload_string(words))) == 2
    assert len(entry.rekey(copy=True)) == 2
    c.load_server_key(b.bsk, _no_ksk())
    _refused(c, lambda: s.download_packed(s.upload_string(words)), "packing key not loaded")
    _refused(c, lambda: entry.rekey(copy=True), "re-key key not loaded")
    _check(c, EXACT, b.out, "8: exact, B")


# ---- c. a compressed key over a plain one ----------------------------------------------------------------------------

def test_a_compressed_key_replaces_a_plain_one_and_a_plain_one_replaces_it(live, keys):
    from fhestring_amd.api import MyClientKey, expand_compressed_server_key
    from oracle import core, radix
    c, (a, b) = live, keys
    c.set_arithmetic(c.ARITH_EXACT_NTT)
    c.load_server_key(b.bsk, _no_ksk())
    _check(c, c.ARITH_F64_FFT, b.m3, "f64, B")                        # the context holds B in both forms
    ck = MyClientKey(0xC5EED)
    try:
        seeded = ck.compressed_server_key()
        osk = core.ServerKey(*expand_compressed_server_key(*seeded))
        names = ["msg", "eq_biv", "sign"]
        luts = np.stack([radix.lut_poly(n) for n in names])
        cts = np.stack([ck.encrypt_char_raw(v)[k] for v in (0x5A, 0xC3, 0xFF) for k in (0, 3)])
        idx = np.arange(len(cts), dtype=np.uint32) % 3
        assert len(cts) == 6
        c.load_compressed_server_key(*seeded)
        assert np.array_equal(c.pbs_batch(cts, idx, luts), osk.pbs_batch(cts, idx, luts, mode=0)), "exact, seeded key"
        c.set_arithmetic(c.ARITH_F64_FFT)
        for fft4_max in (0, 1 << 30):
            c.set_fft4_max_batch(fft4_max)
            got = c.pbs_batch(cts, idx, luts)
            c.set_fft4_max_batch(FFT4_MAX_BATCH_DEFAULT)
            assert np.array_equal(got, osk.pbs_batch(cts, idx, luts, mode=3)), ("f64, seeded key", fft4_max)
    finally:
        ck.close()
    # a plain key over the seeded one, while the f64 arithmetic is selected: item b's outputs are back
    c.load_server_key(a.bsk, _no_ksk())
    _check(c, c.ARITH_F64_FFT, a.m3, "f64, A", b.m3)
    _check(c, c.ARITH_EXACT_NTT, a.out, "exact, A", b.out)
