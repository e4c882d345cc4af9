"""The device check of the packed download of parked store entries on its own: the helper that
smoke() of __graft_entry__.py runs, with a context of its own -- which also covers a context without a packing key.  The
GPU suite is at its cap of `gpu` items, so this file carries no mark: it skips itself unless a device is visible, and
touches none while it is collected."""
import pytest


def test_store_download_on_the_device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import __graft_entry__
    __graft_entry__._smoke_store_download()
