"""The tick scheduler's hazards on the MI355X, word for word against the plan replay (DESIGN.md section 6;
oracle/dag_parity.py scripts H .. L; the conditions that make each script worth running are asserted on the planner in
tests/test_dag_parity.py).

tests/test_gpu_skew.py and tests/test_gpu_lifecycle.py check these paths by decryption, which forgives any error below
2^58 and cannot tell a block from another block with the same message.  Here the strings that the scheduler could
confuse hold the same message under fresh encryptions, and every result is compared in all 4 x 2049 words with the
replay of the planner's trace.  The planner's block tokens are never reused and the replay keeps blocks by token, so it
cannot share a pool-reuse or ordering bug with the device.

    H  the benchmark's schedule in small: six requests, one submitted and one tick pumped per request, each input
       dropped while scheduled levels still have to read it, drained by flush(wait=False): 600 rotations + 468
       extractions.  Tick balance off (groups of three jobs' levels), 48 (every first level split) and the device's
       resident slots (the benchmark's setting); balance 48 in two more kernel configurations
    I  blocks freed under a scheduled tick, and uploads behind them that must not get those blocks: 30 rotations
    J  a job that consumes an unfinished job, a third beside them, two ticks pumped, a flush in between: 124 + 28
    K  fhs_set_auto_flush(16): the ready level peeled 35 times while the DAGs are recorded, a dropped intermediate: 657
    L  two map_clear jobs with random tables: the table array grows in front of the second tick, with the first in the
       stream and two more scheduled: 296 rotations

f64-FFT arithmetic against oracle mode 3; I and J in exact NTT against mode 0 as well, I in the two-bit arithmetics
against modes 4 and 5: the schedule is the same, the kernels behind a launch group and the resident slots are not.  One
fresh device context per test (K needs one that was never driven with submit), one replay per plan.  No tolerance
anywhere.  Like tests/test_dag_parity_device.py this file carries no `gpu` mark: every test skips unless a device is
visible, and none is touched while the file is collected.  Figures are printed per configuration (pytest -s)."""
import pytest

from parity_util import device, replays_or_skip


@pytest.fixture(scope="module")
def replays(oracle_keys, oracle_sk):
    return replays_or_skip(oracle_keys, oracle_sk)


@pytest.mark.parametrize("balance", ["off", "48", "resident"])
def test_one_request_per_tick(replays, balance):
    with device(replays.keys) as sk:
        slots = {"off": 0, "48": 48}[balance] if balance != "resident" else sk.ctx._L.fhs_resident_slots(sk.ctx._h)
        got = replays.check(sk, "H", "f64 FFT, defaults, tick balance %d" % slots, slots=slots)
        assert len(got.plan["launch_groups"]) < len(got.plan["level_widths"])   # rows of several jobs in one group


def test_one_request_per_tick_persistent_kernel_in_launches_of_48(replays):
    with device(replays.keys) as sk:
        sk.ctx.set_fft4_max_batch(0)
        sk.ctx.set_launch_chunk(1, 48)
        replays.check(sk, "H", "f64 FFT, fft4_max_batch 0, launch chunk 48, tick balance 48", slots=48)


def test_one_request_per_tick_four_wavefront_kernel(replays):
    with device(replays.keys) as sk:
        sk.ctx.set_fft4_max_batch(1 << 30)
        replays.check(sk, "H", "f64 FFT, fft4_max_batch 2^30, tick balance 48", slots=48)


@pytest.mark.parametrize("arith", [1, 0, 2, 3])
def test_blocks_freed_under_a_scheduled_tick_are_not_reused_early(replays, arith):
    with device(replays.keys, arith=arith) as sk:
        got = replays.check(sk, "I", "arith %d" % arith)
        assert got.facts["blocks_returned"] == 32, got.facts


@pytest.mark.parametrize("arith", [1, 0])
def test_job_consuming_an_unfinished_job_and_a_flush_in_between(replays, arith):
    with device(replays.keys, arith=arith) as sk:
        replays.check(sk, "J", "arith %d" % arith)


def test_automatic_partial_flush(replays):
    with device(replays.keys) as sk:
        replays.check(sk, "K", "f64 FFT, defaults, auto flush 16")


def test_table_array_grows_under_scheduled_jobs(replays):
    with device(replays.keys) as sk:
        replays.check(sk, "L", "f64 FFT, defaults")
