"""Fused DAGs on the MI355X, word for word against the plan replay (oracle/dag_parity.py).

One script is recorded twice -- on a planner context, whose plan trace the CPU oracle executes with every shared
extraction read from its leader's accumulator (PlanRun(exact_extractions=True)), and on a device context under the same
keys, with the same ciphertexts and the same set_mode / submit / pump / flush calls.  First the guard: both contexts
report the same rotations, extractions, levels, noise figure, level widths and launch groups.  Then every result handle's
download() equals the replay's result_char() in all 4 x 2049 words: level building, lincomb descriptors, the scatter of
outputs, body pointers, extraction descriptors, launch groups, ticks and pool blocks have exactly one right answer.

    A  contains_clear, 64 characters, 4-character pattern: 198 rotations + 366 extractions, levels 130 / 62 / 5 / 1 --
       the first level crosses 128 rows (the keyswitch changes kernels); 304 followers at K >= 2048 (negated)
    B  find (encrypted pattern), flush, char_at + substr at that index, flush: sums as operands across flushes
    C  like_clear with ignore_case, with and without an escape byte: two extractions of one rotation added
    D  le + eq_ignore_case in one flush: negative and multi-term coefficients, shared levels
    E  D and a contains_clear as two submitted jobs, pumped tick by tick with tick balance on
    F  B with the pool compacted between the flushes: moved blocks as operands
    G  as written: eq of two 3-character strings, many narrow levels

f64-FFT arithmetic against oracle mode 3 in three kernel configurations that share one replay per script (none changes
the plan); exact NTT against mode 0 and the two-bit variants against modes 4 and 5 on the smallest shape that shares
rotations.  No tolerance anywhere.  The GPU suite is at its cap of `gpu` items, so this file carries no mark: every test
skips unless a device is visible, and none is touched while the file is collected.  Rotations, extractions and the times
of replay and device run are printed per script and configuration (pytest -s)."""
import pytest

from parity_util import device as _device, replays_or_skip


@pytest.fixture(scope="module")
def replays(oracle_keys, oracle_sk):
    return replays_or_skip(oracle_keys, oracle_sk)


def test_f64_fft_default_kernels(replays):
    with _device(replays.keys) as sk:
        for name in "ABCD":
            replays.check(sk, name, "f64 FFT, defaults")


def test_two_jobs_ride_in_the_same_launch_groups(replays):
    with _device(replays.keys) as sk:
        slots = sk.ctx._L.fhs_resident_slots(sk.ctx._h)          # what set_tick_balance() chooses on this device
        got = replays.check(sk, "E", "f64 FFT, defaults, tick balance %d" % slots, slots=slots)
        assert len(got.plan["launch_groups"]) < len(got.plan["level_widths"])   # rows of both jobs in one group


def test_blocks_moved_by_the_pool_are_read_where_they_are_now(replays):
    with _device(replays.keys) as sk:
        got = replays.check(sk, "F", "f64 FFT, defaults, pool compacted between the flushes")
        assert got.facts["blocks_moved"] > 0, got.facts


def test_every_follower_as_its_own_rotation(replays):
    """rotation sharing off on both contexts: script A's 564 rows each with a rotation of their own"""
    with _device(replays.keys) as sk:
        got = replays.check(sk, "A", "f64 FFT, defaults, rotation sharing off", sharing=False)
        assert got.plan["stats"]["pbs_extracted"] == 0 and got.plan["stats"]["pbs_executed"] == 198 + 366


def test_persistent_kernel_in_launches_of_48(replays):
    """every level through the two-wavefront persistent kernel, 48 ciphertexts a launch: 48 divides neither 130 nor 62,
    followers sit in another launch than their leader"""
    with _device(replays.keys) as sk:
        sk.ctx.set_fft4_max_batch(0)
        sk.ctx.set_launch_chunk(1, 48)
        for name in "AB":
            replays.check(sk, name, "f64 FFT, fft4_max_batch 0, launch chunk 48")


def test_four_wavefront_kernel_at_every_width(replays):
    with _device(replays.keys) as sk:
        sk.ctx.set_fft4_max_batch(1 << 30)
        for name in "AB":
            replays.check(sk, name, "f64 FFT, fft4_max_batch 2^30")


def test_as_written_mode_f64_fft(replays):
    with _device(replays.keys) as sk:
        replays.check(sk, "G", "f64 FFT, defaults, as written")


def test_exact_ntt(replays):
    with _device(replays.keys, arith=0) as sk:
        replays.check(sk, "small", "exact NTT")
        replays.check(sk, "G", "exact NTT, as written")


def test_two_key_bits_per_product(replays):
    from fhestring_amd import Context
    for arith in (Context.ARITH_F64_FFT_MB2, Context.ARITH_EXACT_NTT_MB2):
        with _device(replays.keys, arith=arith) as sk:
            replays.check(sk, "small", "arith %d (two key bits per product)" % arith)


def test_smoke_step(replays):
    import __graft_entry__
    __graft_entry__._smoke_dag_parity(replays.keys, replays.osk)
