"""blind_rotate_fft_kernel (csrc/fft_kernels.hip) with its per-lane twiddles resident across the whole kernel and a 4-point
key window, both instantiations, bit for bit against mode 3 of the CPU oracle (the lane-for-lane mirror) through
fhs_debug_blind_rotate_batch with the 2-wavefront kernel forced.  tests/test_fft_key_window_model.py checks the window's
schedule on paper; here a wrong refill index, a stale twiddle or a window started by a skipped iteration changes output
words.  Six distinct rows, mirrored once per look-up table and shared by every test.

The marked GPU suite is capped (tests/conftest.py, GPU_TEST_CAP) and full.  Like tests/test_pack_synth_device.py and
tests/test_store_synth_device.py this file therefore carries no `gpu` mark: every test skips unless a device is visible,
and none is touched while the file is collected."""
import numpy as np
import pytest

import synth_key as sk

LWE_N = sk.LWE_N
TABLES = ("shifted", "general")


def _mirror(osk, m, lut):
    return sk.sample_extract(osk.blind_rotate(m, lut, mode=3).reshape(2, sk.N))


class Cases:
    pass


@pytest.fixture(scope="module")
def cases(ctx, oracle_sk):
    """Rows 0, 1: every one of the 742 mod-switched mask elements non-zero (no iteration skipped).  Rows 2..5: a zero
    element -- a skipped iteration, which must neither start a key window nor disturb the next one -- at i = 0, at
    i = 741, at two adjacent positions, and right after a non-zero one (and once more further on)."""
    from oracle import radix
    rng = np.random.default_rng(0x4B57)
    ms = rng.integers(1, 4096, (6, LWE_N + 1)).astype(np.uint32)
    ms[2, 0] = 0
    ms[3, 741] = 0
    ms[4, 370:372] = 0
    ms[5, [1, 500]] = 0
    assert (ms[:2, :LWE_N] != 0).all() and ms[5, 0] != 0 and ms[5, 499] != 0
    c = Cases()
    c.ms = ms
    c.ks = ms.astype(np.uint64) << np.uint64(52)
    assert np.array_equal(sk.mod_switch(c.ks), ms)
    clean = radix.lut_poly("eq_biv")                         # a catalogue table: every word a multiple of 2^59
    assert not (clean & np.uint64(0xFF)).any()
    low = rng.integers(1, 256, sk.N).astype(np.uint64)       # a user table with low bytes: the general instantiation
    low[:4] = (0xFF, 0x01, 0x80, 0x7F)
    c.luts = {"shifted": clean, "general": radix.lut_poly("sign") | low}
    c.want = {t: np.stack([_mirror(oracle_sk, m, c.luts[t]) for m in ms]) for t in TABLES}
    for a in c.want.values():
        a.setflags(write=False)
    assert not np.array_equal(c.want["shifted"], c.want["general"])
    return c


@pytest.fixture(scope="module")
def ctx(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import fhestring_amd
    oracle_keys = request.getfixturevalue("oracle_keys")
    c = fhestring_amd.Context(0)
    c.set_arithmetic(c.ARITH_F64_FFT)
    c.load_server_key(oracle_keys.bsk, oracle_keys.ksk)
    c.set_fft4_max_batch(0)                                  # every batch on the 2-wavefront kernel
    yield c
    c.close()


def _run(ctx, cases, table, rows):
    """The rows through the 2-wavefront kernel with one table; checks which instantiation the launch ran."""
    wide, shifted = ctx.kernel_timing_kind(0)[1:], ctx.kernel_timing_kind(3)[1:]
    got = ctx.blind_rotate_batch(cases.ks[rows], np.zeros(len(rows), np.uint32), cases.luts[table][None])
    assert tuple(np.subtract(ctx.kernel_timing_kind(0)[1:], wide)) == (1, len(rows))
    assert tuple(np.subtract(ctx.kernel_timing_kind(3)[1:], shifted)) == ((1, len(rows)) if table == "shifted" else (0, 0))
    return got


def _bad(got, want, rows):
    return [(b, int(rows[b])) for b in range(len(rows)) if not np.array_equal(got[b], want[rows[b]])]


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_rows_through_all_742_iterations(ctx, cases, B, table):
    """The smallest shapes at which a wrong refill index or a stale twiddle shows."""
    rows = np.arange(B)
    assert _bad(_run(ctx, cases, table, rows), cases.want[table], rows) == []


@pytest.mark.parametrize("table", TABLES)
def test_skipped_iterations_leave_the_key_window_alone(ctx, cases, table):
    rows = np.arange(2, 6)
    assert _bad(_run(ctx, cases, table, rows), cases.want[table], rows) == []


@pytest.mark.parametrize("table", TABLES)
def test_more_rows_than_resident_workgroups(ctx, cases, table):
    """slots + 3 rows: at least three workgroups take a second ciphertext from the counter, with the twiddles they loaded
    before the first.  The rows repeat the six distinct ones, so every row -- the first, the last, those taken second --
    is compared with the mirror; and all of them with the 4-wavefront kernel."""
    slots = ctx._L.fhs_resident_slots(ctx._h)
    rows = np.arange(slots + 3) % len(cases.ms)
    got = _run(ctx, cases, table, rows)
    assert _bad(got, cases.want[table], rows) == []
    ctx.set_fft4_max_batch(1 << 30)
    try:
        other = ctx.blind_rotate_batch(cases.ks[rows], np.zeros(len(rows), np.uint32), cases.luts[table][None])
    finally:
        ctx.set_fft4_max_batch(0)
    assert np.array_equal(got, other)
