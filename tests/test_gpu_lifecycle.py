"""Lifetime of a context's HIP resources on the MI355X: every device allocation, pinned buffer, event and stream has one
owner, fhs_ctx_destroy is a delete, and fhs_debug_live_resources counts what this library holds -- so "nothing is left"
is asserted exactly, whatever else runs on the device.  f64-FFT arithmetic, fused mode, one client key for the module;
the shapes are the smallest that reach each path (4 blocks: the staged upload at its minimum size; 264 blocks: one more
than the transfer buffer's 260-row minimum, so it regrows)."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ck():
    from fhestring_amd.api import MyClientKey
    k = MyClientKey(1212)
    k.packing_key()
    yield k
    k.close()


def _server(ck, packing_key=True):
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.from_client_key(ck, arith=1)
    sk.set_mode(1)
    if packing_key:
        sk.load_packing_key(ck)
    return sk


def _live():
    from fhestring_amd._lib import live_resources
    return live_resources()


def _nothing_left():
    gc.collect()                                     # contexts of earlier modules that nothing refers to any more
    live = _live()
    assert live[:4] == [0, 0, 0, 0], live
    return live


def test_create_use_destroy_three_times(ck):
    """Per cycle: both keys, a 1-character upload (4 blocks, staged), a 66-character upload (264 blocks: the transfer buffer
    regrows while its first copy's event exists), one character block by block, to_upper and eq, plain and packed
    download, the store's put / get of a window / export / import / drop -- everything decrypted and compared; after
    each close() the library holds nothing, and every cycle acquired something."""
    rng = np.random.default_rng(12)
    acquired = _nothing_left()[4]
    for cycle in range(3):
        text = "".join(chr(c) for c in rng.integers(33, 127, 66))
        sk = _server(ck)
        one = sk.upload_string(ck.encrypt_str_raw("q", 0))
        long = sk.upload_string(ck.encrypt_str_raw(text, 0))
        twin = sk.upload_string(ck.encrypt_str_raw("q", 0))
        single = sk.upload_char(ck.encrypt_char_raw(ord("k")))
        held = _live()
        assert held[0] > 0 and held[1] > 0 and held[2] > 0 and held[3] == 1, held
        up = sk.to_upper(long)
        same = sk.eq(one, twin)
        sk.flush()
        assert ck.decrypt(up) == text.upper(), cycle
        assert ck.decrypt_char(same) == 1 and ck.decrypt_char(single) == ord("k") and ck.decrypt(one) == "q", cycle
        assert ck.decrypt_packed(sk.download_packed(up)) == text.upper(), cycle
        e = sk.store_put(up)
        assert ck.decrypt(e.get(60, 3)) == text.upper()[60:63], cycle
        compact, meta = e.export()
        imp = sk.store_import(compact, meta)
        assert ck.decrypt(imp.get()) == text.upper(), cycle
        e.drop()
        imp.drop()
        sk.close()
        live = _nothing_left()
        assert live[4] > acquired, (cycle, live)
        acquired = live[4]


def test_block_freed_under_a_scheduled_tick_is_not_reused_early(ck):
    """The inputs of a submitted job are released before any pump; the uploads of B and C are in the stream before that
    job's tick is, so they must not get its input blocks.  to_upper's result still refers to A's blocks (the untouched
    blocks are shared, the changed one is a sum with the flag), so releasing A returns nothing to the pool; the eq of D1 and
    D2 in the same job is a bootstrap output of its own, and its 32 input blocks do go back under the scheduled tick.  If
    they were handed to B and C (which differ), D's flag would read 0."""
    sk = _server(ck, packing_key=False)
    try:
        a = sk.upload_string(ck.encrypt_str_raw("abcd", 0))
        d1 = sk.upload_string(ck.encrypt_str_raw("mnop", 0))
        d2 = sk.upload_string(ck.encrypt_str_raw("mnop", 0))
        up = sk.to_upper(a)
        same_d = sk.eq(d1, d2)
        sk.submit()
        live = sk.stats()["blocks_live"]
        del a, d1, d2
        assert sk.stats()["blocks_live"] == live - 32
        b = sk.upload_string(ck.encrypt_str_raw("wxyz", 0))
        c = sk.upload_string(ck.encrypt_str_raw("wxyq", 0))
        same = sk.eq(b, c)
        sk.submit()
        sk.flush()
        assert ck.decrypt(up) == "ABCD"
        assert ck.decrypt_char(same_d) == 1
        assert ck.decrypt_char(same) == 0
    finally:
        sk.close()
    _nothing_left()


def test_destroy_with_work_outstanding(ck):
    """A submitted job that was never pumped, a parked store entry and live handles: close() returns and frees it all."""
    sk = _server(ck)
    s = sk.upload_string(ck.encrypt_str_raw("park", 0))
    entry = sk.store_put(s)
    up = sk.to_upper(s)
    sk.submit()
    assert sk.store_stats()["entries"] == 1 and _live()[0] > 0
    sk.close()
    _nothing_left()
    del up, entry, s                                                             # handles outlive their context harmlessly


def test_two_contexts_on_one_device(ck):
    first, second = _server(ck, packing_key=False), _server(ck, packing_key=False)
    assert _live()[3] == 2
    u1 = first.to_upper(first.upload_string(ck.encrypt_str_raw("left", 0)))
    u2 = second.to_upper(second.upload_string(ck.encrypt_str_raw("both", 0)))
    r1, r2 = ck.decrypt(u1), ck.decrypt(u2)
    first.close()
    live = _live()
    assert live[0] > 0 and live[3] == 1, live
    assert ck.decrypt(u2) == "BOTH"                                               # the survivor is untouched
    second.close()
    assert (r1, r2) == ("LEFT", "BOTH")
    _nothing_left()


def test_failed_creation_is_destroyed_like_any_other():
    from fhestring_amd._lib import lib
    L = lib()
    before = _nothing_left()
    h = C.c_void_p()
    rc = L.fhs_ctx_create(9999, C.byref(h))                                       # beyond any device count
    assert rc != 0 and h.value
    assert b"device_id out of range" in L.fhs_last_error(h)
    L.fhs_ctx_destroy(h)
    after = _nothing_left()
    assert after[4] == before[4]                                                  # it never got as far as a resource
