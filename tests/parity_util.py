"""Shared by the device halves of the word-for-word comparison (tests/test_dag_parity_device.py,
tests/test_sched_parity_device.py): the replays of a module, and a device context under the oracle's keys."""
import contextlib


class Replays:
    """the module's replays, each made when first asked for and shared by every configuration that runs its plan"""

    def __init__(self, keys, osk):
        self.keys, self.osk, self._cases, self._done = keys, osk, {}, {}
        osk.set_mb2(keys.bsk_mb2)

    def case(self, name):
        from oracle import dag_parity
        if name not in self._cases:
            self._cases[name] = dag_parity.case(name, self.keys)
        return self._cases[name]

    def want(self, name, mode, sharing=True, **extra):
        from oracle import dag_parity
        key = (name, mode, sharing, tuple(sorted(extra.items())))
        if key not in self._done:
            script, string_mode, inputs = self.case(name)
            self._done[key] = dag_parity.replay(script, dict(inputs, **extra), self.osk, mode, string_mode, sharing)
        return self._done[key]

    def check(self, sk, name, config, sharing=True, **extra):
        """guard, then every word; -> the device's Outcome"""
        from oracle import dag_parity
        mode = dag_parity.ORACLE_MODE[sk.ctx.arithmetic]
        want = self.want(name, mode, sharing, **extra)
        script, string_mode, inputs = self.case(name)
        what = "script %s, %s" % (name, config)
        got = dag_parity.check(script, dict(inputs, **extra), want, sk, what, string_mode=string_mode, sharing=sharing)
        print("%s: %d rotations + %d extractions in %d launch groups, guard held, %d results equal in every word; "
              "replay %.2f s (oracle mode %d), device %.3f s" % (what, want.rotations, want.extractions,
                                                                len(want.plan["launch_groups"]), len(want.words),
                                                                want.seconds, mode, got.seconds))
        return got


def replays_or_skip(oracle_keys, oracle_sk):
    """what a module's `replays` fixture returns; nothing touches the device before a test asks for this"""
    import pytest
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return Replays(oracle_keys, oracle_sk)


@contextlib.contextmanager
def device(keys, arith=1):
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.from_raw_keys(keys.bsk, keys.ksk, arith=arith, bsk_mb2=keys.bsk_mb2 if arith in (2, 3) else None)
    try:
        yield sk
    finally:
        sk.close()
