"""The device checks of seeded select queries, the query conversion kernel and several queries per call (DESIGN.md section
24): the helpers that smoke() of __graft_entry__.py runs as its step 15, on one context of this module.  The GPU suite is
at its cap of `gpu` items, so this file carries no mark: it skips itself unless a device is visible, and touches none while
it is collected."""
import pytest


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from fhestring_amd.api import MyClientKey, MyServerKey
    a = MyClientKey(0x5EEDA)
    sk = MyServerKey.from_client_key(a)
    sk.load_packing_key(a)                                   # (put packs the table of the end-to-end test)
    yield sk, a
    sk.close()
    a.close()


def test_query_conversion_equals_the_host_bit_for_bit(env):
    import __graft_entry__
    __graft_entry__._select_seeded_conversion(env[0])


def test_seeded_select_equals_the_host_on_the_expanded_query(env):
    import __graft_entry__
    __graft_entry__._select_seeded_words(env[0])


def test_batches_equal_single_calls_and_the_host(env):
    import __graft_entry__
    __graft_entry__._select_seeded_batch(env[0])


def test_select_many_end_to_end(env):
    import __graft_entry__
    __graft_entry__._select_seeded_flow(*env)


def test_diagnostics_refuse_a_planner_and_a_context_without_tables():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import numpy as np
    from fhestring_amd import Context, FhsError
    from fhestring_amd.api import MyServerKey
    q = np.zeros((1, 4, 2, 2048), np.uint64)
    bare = Context(0)                                        # no server key yet: no transform tables on the device
    try:
        with pytest.raises(FhsError) as err:
            bare.select_query_device(q)
        assert err.value.code == -3
    finally:
        bare.close()
    plan = MyServerKey.planner()
    try:
        with pytest.raises(FhsError) as err:
            plan.ctx.select_query_device(q)
        assert err.value.code == -3
    finally:
        plan.close()
