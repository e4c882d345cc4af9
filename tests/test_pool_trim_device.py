"""The device check of block pool accounting and trimming on its own: the helper that smoke() of
__graft_entry__.py runs, with a context of its own -- release, compaction on the GPU in one and in two passes of moves,
every surviving word compared, a moved string used as an operand, trims with work outstanding.  The GPU suite is at its
cap of `gpu` items, so this file carries no mark: it skips itself unless a device is visible, and touches none while it
is collected."""
import pytest


def test_pool_trim_on_the_device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import __graft_entry__
    __graft_entry__._smoke_pool_trim()
