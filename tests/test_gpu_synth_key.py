"""The six blind-rotation kernels under the synthetic monomial keys of tests/synth_key.py, against integer numpy
references that use no transform at all (anchored to the oracle's schoolbook product by tests/test_synth_key.py), on a
row set whose look-up tables put exact decomposition ties into every product: the exact kernels bit for bit, the f64
kernels bit for bit against their mirrors and within T3 / T4 of the integer reference on one-product rows.  The same
under keys with dense full-magnitude GGSWs, near the top of the exact kernels' CRT range.  And the keyswitch under a
synthetic key that brings every byte plane of every key word to a modulus-switch edge, on every launch shape."""
import numpy as np
import pytest

import synth_key as sk

pytestmark = pytest.mark.gpu

# The library's default of fhs_set_fft4_max_batch (fhestring_amd/api.py: Context.set_fft4_max_batch); the C ABI has a
# setter only, so the value is restated here like in tests/test_gpu_kat.py and restored after every forced route.
FFT4_MAX_BATCH_DEFAULT = 512


@pytest.fixture(scope="module")
def mat():
    return sk.material()


@pytest.fixture(scope="module")
def ref():
    return sk.references()


@pytest.fixture(scope="module")
def ctx(mat):
    import fhestring_amd
    c = fhestring_amd.Context(0)
    c.set_arithmetic(c.ARITH_F64_FFT)                 # builds the Fourier-domain key beside the residues
    c.load_server_key(mat.bsk, sk.keyswitch_material().ksk)             # the blind-rotation entry never keyswitches
    c.load_multibit_key(mat.bsk_mb2)
    c.set_arithmetic(c.ARITH_EXACT_NTT)
    c.load_multibit_key(mat.bsk_mb2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def osk(mat):
    from oracle import core
    return core.ServerKey(mat.bsk, np.zeros(core.KSK_WORDS, np.uint64)).set_mb2(mat.bsk_mb2)


def _mirror(osk, ms, luts, lut_idx, mode):
    """Extracted outputs of an oracle mode, once per distinct row."""
    return np.stack([sk.sample_extract(osk.blind_rotate(ms[r], luts[lut_idx[r]], mode=mode).reshape(2, sk.N))
                     for r in range(len(ms))])


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


def test_exact_ntt_kernel_equals_the_integer_reference(ctx, mat, ref):
    for n in (None, 300):
        got, src = _run(ctx, ctx.ARITH_EXACT_NTT, mat.ks, mat.lut_idx, mat.luts, n)
        assert _bad(got, src, ref.out) == [], n


def test_f64_fft_kernels_equal_their_mirror_and_stay_within_t3_of_the_integer_reference(ctx, mat, ref, osk):
    want = _mirror(osk, mat.ms, mat.luts, mat.lut_idx, 3)
    single = sk.rows_of(mat, "single")
    # Which 4-wavefront variant a forced launch runs is decided by launch_blind_rotate_fft4 alone: B * 4 <= slots (4 per
    # CU) -> the wide-LDS variant, more -> the shared-area variant.  The widths follow the context's own slot count, so
    # that a device with fewer CUs cannot send both launches to the same variant unnoticed.
    ctx.set_arithmetic(ctx.ARITH_F64_FFT)
    slots = ctx._L.fhs_resident_slots(ctx._h)
    ctx.set_arithmetic(ctx.ARITH_EXACT_NTT)
    assert 4 * len(mat.ks) <= slots, "the row set no longer fits the wide-LDS variant of the 4-wavefront kernel"
    n_shared, n_rounds = max(300, slots // 4 + 1), max(1056, slots + 32)
    # 2 wavefronts; 4 wavefronts, wide-LDS variant; 4 wavefronts, shared-area variant; 2 wavefronts again with more than
    # one round of the persistent workgroups (one per slot)
    for fft4_max, n in ((0, None), (1 << 30, None), (1 << 30, n_shared), (0, n_rounds)):
        got, src = _run(ctx, ctx.ARITH_F64_FFT, mat.ks, mat.lut_idx, mat.luts, n, fft4_max)
        assert _bad(got, src, want) == [], (fft4_max, n)
        worst = max(sk.centred_abs_max(got[r], ref.out[r]) for r in single)
        assert worst < sk.T3, (fft4_max, n, worst)


def test_exact_two_bit_kernel_equals_the_integer_reference(ctx, mat, ref):
    for n in (None, 300):
        got, src = _run(ctx, ctx.ARITH_EXACT_NTT_MB2, mat.ks, mat.lut_idx, mat.luts, n)
        assert _bad(got, src, ref.out_mb2) == [], n


def test_f64_two_bit_kernel_equals_its_mirror_and_stays_within_t4_of_the_integer_reference(ctx, mat, ref, osk):
    want = _mirror(osk, mat.ms, mat.luts, mat.lut_idx, 4)
    for n in (None, 300):
        got, src = _run(ctx, ctx.ARITH_F64_FFT_MB2, mat.ks, mat.lut_idx, mat.luts, n)
        assert _bad(got, src, want) == [], n
        worst = max(sk.centred_abs_max(got[r], ref.out_mb2[r]) for r in sk.rows_of(mat, "single", "pair"))
        assert worst < sk.T4, (n, worst)


def test_chosen_masks_and_edge_luts_under_the_real_dense_key(mat, oracle_keys, oracle_sk):
    """Exact ties in the first product under a key with full-magnitude dense coefficients: the exact kernel against
    oracle mode 0 (== schoolbook on these rows, tests/test_synth_key.py), both f64 routes against mode 3."""
    import fhestring_amd
    ks, ms, lut_idx = sk.dense_case()
    want0 = _mirror(oracle_sk, ms, mat.luts, lut_idx, 0)
    want3 = _mirror(oracle_sk, ms, mat.luts, lut_idx, 3)
    c = fhestring_amd.Context(0)
    try:
        c.set_arithmetic(c.ARITH_F64_FFT)
        c.load_server_key(oracle_keys.bsk, oracle_keys.ksk)
        got, src = _run(c, c.ARITH_EXACT_NTT, ks, lut_idx, mat.luts)
        assert _bad(got, src, want0) == []
        for fft4_max in (0, 1 << 30):
            got, src = _run(c, c.ARITH_F64_FFT, ks, lut_idx, mat.luts, None, fft4_max)
            assert _bad(got, src, want3) == [], fft4_max
    finally:
        c.close()


def test_keyswitch_under_the_synthetic_key_on_every_launch_shape(ctx):
    """Every row of every width against the integer reference (== the oracle in all 64 bits, tests/test_synth_key.py).
    On the edge rows all 743 outputs sit on a modulus-switch edge or one unit beside it, so one wrong unit in any byte
    plane shows.  The widths are the smallest that reach each launch shape of launch_keyswitch_mfma on 256 CUs; on a
    part where a width gets another shape it is left out rather than passed off as that shape."""
    m = sk.keyswitch_material()
    want = sk.mod_switch(sk.keyswitch_reference())
    cus = ctx._L.fhs_resident_slots(ctx._h) // 2              # exact arithmetic: 2 workgroups per CU
    widths = [w for w in sk.KS_WIDTHS if sk.ks_launch_shape(w, cus) == sk.KS_SHAPES_256[w]]
    assert cus != 256 or widths == list(sk.KS_WIDTHS)
    for width in widths:
        src = sk.ks_batch(width)
        got = ctx.keyswitch_modswitch_batch(m.cts[src])
        bad = np.flatnonzero((got != want[src]).any(axis=1))
        assert bad.size == 0, ("width", width, sk.KS_SHAPES_256[width], "first bad (batch row, distinct row, kind)",
                               [(int(b), int(src[b]), m.kinds[src[b]]) for b in bad[:8]])


def test_every_kernel_on_the_extreme_rows_near_the_top_of_the_crt_range():
    """Keys with dense GGSWs of full-magnitude coefficients, constant look-up tables, digits of -2^22 in every
    coefficient: product coefficients of 2^90 to 2^91 (classic) and 2^91 to 2^92 (two-bit) in grid units, against a CRT
    range of 2^93.  The exact kernels against the integer references bit for bit, the f64 kernels against their mirrors
    bit for bit and within T3X / T4X of the integer references on the rows that end in their one dense product."""
    import fhestring_amd
    from oracle import core
    x, ref = sk.extreme_material(), sk.extreme_references()
    osk = core.ServerKey(x.bsk, np.zeros(core.KSK_WORDS, np.uint64)).set_mb2(x.bsk_mb2)
    want3, want4 = _mirror(osk, x.ms, x.luts, x.lut_idx, 3), _mirror(osk, x.ms, x.luts, x.lut_idx, 4)
    c = fhestring_amd.Context(0)
    try:
        c.set_arithmetic(c.ARITH_F64_FFT)
        c.load_server_key(x.bsk, np.zeros(core.KSK_WORDS, np.uint64))
        c.load_multibit_key(x.bsk_mb2)
        c.set_arithmetic(c.ARITH_EXACT_NTT)
        c.load_multibit_key(x.bsk_mb2)
        for n in (None, 300):
            got, src = _run(c, c.ARITH_EXACT_NTT, x.ks, x.lut_idx, x.luts, n)
            assert _bad(got, src, ref.out) == [], ("exact", n)
            got, src = _run(c, c.ARITH_EXACT_NTT_MB2, x.ks, x.lut_idx, x.luts, n)
            assert _bad(got, src, ref.out_mb2) == [], ("exact two-bit", n)
            got, src = _run(c, c.ARITH_F64_FFT_MB2, x.ks, x.lut_idx, x.luts, n)
            assert _bad(got, src, want4) == [], ("f64 two-bit", n)
            worst = max(sk.centred_abs_max(got[r], ref.out_mb2[r]) for r in x.one_dense_mb2)
            assert worst < sk.T4X, ("f64 two-bit", n, worst)
        # 2 wavefronts; 4 wavefronts, wide-LDS variant; 4 wavefronts, shared-area variant (see the monomial-key item)
        c.set_arithmetic(c.ARITH_F64_FFT)
        slots = c._L.fhs_resident_slots(c._h)
        c.set_arithmetic(c.ARITH_EXACT_NTT)
        assert 4 * len(x.ks) <= slots
        for fft4_max, n in ((0, None), (1 << 30, None), (1 << 30, max(300, slots // 4 + 1))):
            got, src = _run(c, c.ARITH_F64_FFT, x.ks, x.lut_idx, x.luts, n, fft4_max)
            assert _bad(got, src, want3) == [], ("f64", fft4_max, n)
            worst = max(sk.centred_abs_max(got[r], ref.out[r]) for r in x.one_dense)
            assert worst < sk.T3X, ("f64", fft4_max, n, worst)
    finally:
        c.close()
