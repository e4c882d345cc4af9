"""The device check of like_clear on its own: the helper that smoke() of __graft_entry__.py runs,
with a context of its own -- fused and as written, every result decrypted against the regular expression of its pattern,
one result used as an operand, the noise bookkeeping at the end.  The GPU suite is at its cap of `gpu` items, so this file
carries no mark: it skips itself unless a device is visible, and touches none while it is collected."""
import pytest


def test_like_on_the_device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import __graft_entry__
    __graft_entry__._smoke_like()
