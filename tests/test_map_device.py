"""The device check of user tables, map_clear, class_flags, find_class and count_class on its own:
the helper that smoke() of __graft_entry__.py runs, with a context of its own -- the device copies of the user tables
against the host's polynomials, results decrypted against bytes.translate and Python's membership test, one result as an
operand, a table registered on a live context, one result word for word against the plan replay.  The GPU suite is at
its cap of `gpu` items, so this file carries no mark: it skips itself unless a device is visible, and touches none while
it is collected."""
import pytest


def test_map_on_the_device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import __graft_entry__
    __graft_entry__._smoke_map()
