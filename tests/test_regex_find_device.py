"""The device check of regex_find_clear / regex_find_clear_wide / regex_starts_clear on its own: the
helper that smoke() of __graft_entry__.py runs last, with a context of its own -- fused and as written, every position and
flag decrypted against Python's `re`, flags and a position used as operands, the wide form past 256 characters, the noise
bookkeeping, and one fused position word for word against the replay of its plan.  The GPU suite is at its cap of `gpu`
items, so this file carries no mark: it skips itself unless a device is visible, and touches none while it is collected."""
import pytest


def test_regex_find_on_the_device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import __graft_entry__
    __graft_entry__._smoke_regex_find()
