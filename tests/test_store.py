"""Device-resident string store on the host (include/fhestring_hip.h, "device-resident string store"; DESIGN.md section
13): the 32-bit storage switch against numpy, the round trip pack_host -> pack_switch32 -> CompactFheString.expand ->
decryption with its windows, the noise a restored block carries, and -- on a planner context, which records the store's
bookkeeping exactly as a device context does -- the noise figures, the rotation groups and the cycle limit across put /
get, the entry table and the export format.  The device side is tests/test_gpu_store.py."""
import ctypes as C
import math
import random

import numpy as np
import pytest

from ring_util import block_phases, round32

N = 2048
BIG_CT = 2049
GLWE_NOISE = 2.9403601535432533e-16          # client.cpp: GLWE noise as a fraction of the torus (packing key, fresh blocks)
PACK_BASE_LOG, PACK_LEVELS = 16, 3
FHS_ERR_ARG, FHS_ERR_STATE, FHS_ERR_LIMIT = -1, -3, -4
MAX_CYCLES = 16
TR_UPLOAD = 1


@pytest.fixture(scope="module")
def ck():
    from fhestring_amd.api import MyClientKey
    k = MyClientKey(4242)
    yield k
    k.close()


@pytest.fixture()
def sk():
    from fhestring_amd.api import MyServerKey
    s = MyServerKey.planner()
    s.set_auto_flush(0)
    yield s
    s.close()


def _ascii(rng, n):
    return "".join(chr(rng.randrange(1, 128)) for _ in range(n))


def _block_values(blocks, glwe_sk):
    """value mod 32 of every block: the phase rounded to the 2^59 grid"""
    return (((block_phases(blocks, glwe_sk) + np.uint64(1 << 58)) >> np.uint64(59)) & np.uint64(31)).astype(np.uint8)


def _predicted_pack_sigma():
    """V_ks (N^2 - 1) / 3 plus the pre-scaling's N^2 (1 + N / 2) / 12"""
    s2 = (GLWE_NOISE * 2.0 ** 64) ** 2
    v_ks = PACK_LEVELS * N * (2.0 ** (2 * PACK_BASE_LOG) / 12) * s2 + (N / 2) * 2.0 ** (2 * (64 - PACK_LEVELS * PACK_BASE_LOG)) / 12
    return math.sqrt(v_ks * (N * N - 1) / 3 + N * N * (1 + N / 2) / 12)


def _put_raw(sk, chars):
    from fhestring_amd.api import _harr
    eid = C.c_uint64(0)
    rc = sk.ctx._L.fhs_store_put(sk.ctx._h, _harr(chars), len(chars), C.byref(eid))
    return rc, eid.value


def _trace(sk):
    """the plan trace recorded since the last read (reading clears it)"""
    n = C.c_size_t()
    sk.ctx._check(sk.ctx._L.fhs_debug_plan_read(sk.ctx._h, None, 0, C.byref(n)))
    buf = np.zeros(max(1, n.value), np.uint64)
    sk.ctx._check(sk.ctx._L.fhs_debug_plan_read(sk.ctx._h, buf.ctypes.data, n.value, C.byref(n)))
    return buf[:n.value]


def test_switch32_equals_numpy_in_every_word():
    from fhestring_amd.api import CompactFheString, pack_switch32
    rng = np.random.default_rng(11)
    for n_blocks in (4, 2048, 2052):
        g = (n_blocks + N - 1) // N
        m64 = rng.integers(0, 1 << 64, (g, N), dtype=np.uint64)
        b64 = rng.integers(0, 1 << 64, (g, N), dtype=np.uint64)
        m64[0, :4] = [0, (1 << 31) - 1, 1 << 31, (1 << 64) - 1]                  # the rounding's edges, the wrap to 0 included
        m64[-1, 4:6] = [0xFFFFFFFF7FFFFFFF, 0xFFFFFFFF80000000]                  # ... and both sides of the wrap, in the last group
        b64[-1, :4] = [0x000000007FFFFFFF, 0x0000000080000000, 0xFFFFFFFF7FFFFFFF, 0xFFFFFFFF80000000]   # the bodies' too
        c = pack_switch32(m64, b64, n_blocks)
        assert isinstance(c, CompactFheString) and len(c) == n_blocks // 4
        assert c.mask32.shape == (g, N) and c.body32.shape == (n_blocks,)
        assert np.array_equal(c.mask32, round32(m64)), n_blocks
        assert list(c.mask32[0, :4]) == [0, 0, 1, 0] and list(c.mask32[-1, 4:6]) == [0xFFFFFFFF, 0]
        assert list(c.body32[(g - 1) * N:(g - 1) * N + 4]) == [0, 1, 0xFFFFFFFF, 0]
        assert np.array_equal(c.body32, round32(b64).reshape(-1)[:n_blocks]), n_blocks   # group g's bodies start at 2048 g
    m32, b32 = pack_switch32(m64[:1], b64[:1], 3)                               # not whole characters: the raw arrays
    assert np.array_equal(m32, round32(m64[:1])) and np.array_equal(b32, round32(b64[0, :3]))


def test_round_trip_and_windows(ck):
    """1, 512 and 513 characters (4, 2048 and 2052 blocks) with paddings 0 / 1 / 7 through pack_host -> pack_switch32 ->
    expand -> classic decryption; windows across the group boundary and inside a workgroup's eight coefficients equal the
    same rows of the full expansion; block values with carries come back block by block."""
    from fhestring_amd.api import pack_host, pack_switch32
    rng = random.Random(5)
    key = ck.packing_key()
    _, glwe_sk = ck.secret_keys()
    for total in (1, 512, 513):
        for padding in (0, 1, 7):
            if padding > total:
                continue
            text = _ascii(rng, total - padding)
            ct = ck.encrypt_str_raw(text, padding)
            c = pack_switch32(*pack_host(key, ct), 4 * total)
            full = c.expand()
            assert full.shape == (total, 4, BIG_CT)
            assert ck.decrypt_str_raw(full) == ck.decrypt_str_raw(ct) == text, (total, padding)
            if padding == 0:
                for first, count in ((510, 3), (1, 1), (512, 1)):
                    if first + count <= total:
                        assert np.array_equal(c.expand(first, count), full[first:first + count]), (total, first, count)
    vals = np.array(list(range(16)) * 2, np.uint8)
    c = pack_switch32(*pack_host(key, ck.encrypt_blocks_raw(vals)), len(vals))
    assert np.array_equal(_block_values(c.expand(), glwe_sk), vals)


def test_noise_of_restored_blocks(ck):
    """2048 fresh blocks parked and restored on the host: the phase error of the restored blocks is the packing noise of
    DESIGN.md section 11 plus the 32-bit rounding, sigma_32 = 2^32 sqrt((1 + |S|^2) / 12), which disappears under it."""
    from fhestring_amd.api import pack_host, pack_switch32
    rng = np.random.default_rng(3)
    vals = rng.integers(0, 16, 2048).astype(np.uint8)
    blocks = ck.encrypt_blocks_raw(vals)
    restored = pack_switch32(*pack_host(ck.packing_key(), blocks), 2048).expand()
    _, glwe_sk = ck.secret_keys()
    want = vals.astype(np.uint64) << np.uint64(59)
    err = (block_phases(restored, glwe_sk) - want).view(np.int64).astype(np.float64)
    sigma_pack = _predicted_pack_sigma()
    sigma_32 = 2.0 ** 32 * math.sqrt((1 + float(glwe_sk.sum())) / 12)
    predicted = math.sqrt(sigma_pack ** 2 + sigma_32 ** 2)
    sigma = float(err.std())
    print("restored blocks: sigma 2^%.2f, derived 2^%.2f (packing 2^%.2f, 32-bit rounding 2^%.2f), max |e| 2^%.2f" %
          (math.log2(sigma), math.log2(predicted), math.log2(sigma_pack), math.log2(sigma_32), math.log2(np.abs(err).max())))
    assert predicted / 2 < sigma < predicted * 2
    assert sigma < 2.0 ** 46


def test_planner_put_get_and_one_upload_per_block(sk):
    s = sk.dummy_string(5)
    sk.ctx._check(sk.ctx._L.fhs_debug_plan_trace(sk.ctx._h, 1))
    live = sk.stats()["blocks_live"]
    e = sk.store_put(s)
    assert e.id != 0 and len(e) == 5 and sk.stats()["blocks_live"] == live       # the planner allocates nothing for an entry
    _trace(sk)
    w = e.get(1, 3)
    t = _trace(sk)
    assert len(w) == 3 and sk.stats()["blocks_live"] == live + 12
    assert t.size == 2 * 12 and list(t[0::2]) == [TR_UPLOAD] * 12 and len(set(t[1::2].tolist())) == 12
    assert len(e.get()) == 5 and len(e.get(5, 0)) == 0
    res = sk.contains_clear(e.get(), "ab")                                       # restored characters are ordinary operands
    sk.flush()
    assert res.sum_c2() <= 4 and sk.stats()["pbs_executed"] > 0


def test_noise_figures_survive_parking(sk):
    """fhs_char_sum_c2 of a restored character is the figure before put: an upload (1), an upload declared noisier (9), a
    fused-mode if_then_else result (a sum of two bootstrap outputs per block), and a trivial character, which comes back
    as an ordinary ciphertext."""
    from fhestring_amd.api import FheString
    sk.set_mode(1)
    a, b, c, d = sk.dummy_string(4).chars
    b.set_noise(9)
    sel = a.eq(c).if_then_else(c, d)
    triv = sk.trivial(ord("x"))
    before = [h.sum_c2() for h in (a, b, sel, triv)]
    assert before[:2] == [1, 9] and before[2] > 1 and before[3] == 0
    e = sk.store_put(FheString([a, b, sel, triv]))
    back = e.get()
    assert [h.sum_c2() for h in back.chars] == [1, 9, before[2], 1]
    assert [h.sum_c2() for h in (a, b, sel, triv)] == before                     # the parked handles keep theirs
    assert back[3].trivial_value() is None and triv.trivial_value() == ord("x")  # constant folding does not survive parking
    assert e.get(2, 1)[0].sum_c2() == before[2]                                  # by window as well
    # a block above 4 is refreshed on its way into the next operator, restored or not
    sk.stats(reset=True)
    r = back[1].eq(back[0])
    sk.flush()
    assert r.sum_c2() <= 4 and sk.stats()["max_input_sum_c2"] <= 64


def test_cycle_limit(sk):
    """16 put / get cycles of one string succeed, the 17th put is refused; any bootstrap starts the count again.  In the
    as-written mode to_upper bootstraps every block; in fused mode it bootstraps none of the character's own blocks (it
    adds a flag to one of them), so the count rightly stays."""
    from fhestring_amd.api import FheString
    s = sk.dummy_string(3)
    for cycle in range(MAX_CYCLES):
        e = sk.store_put(s)
        s = e.get()
        e.drop()
    rc, eid = _put_raw(sk, s.chars)
    assert rc == FHS_ERR_LIMIT and eid == 0 and sk.store_stats()["entries"] == 0
    assert [h.sum_c2() for h in s.chars] == [1, 1, 1]                            # the integer figure cannot show the packings
    # a sum takes the largest count of its terms: one block of 16 cycles poisons it
    sk.set_mode(1)
    fresh = sk.dummy_string(2)
    mixed = fresh[0].eq(fresh[1]).if_then_else(fresh[0], fresh[1])               # bootstrap outputs only: count 0
    assert _put_raw(sk, [mixed])[0] == 0
    up_fused = sk.to_upper(s)
    sk.flush()
    assert _put_raw(sk, up_fused.chars)[0] == FHS_ERR_LIMIT
    sk.set_mode(0)
    up = sk.to_upper(s)
    sk.flush()
    for cycle in range(MAX_CYCLES):
        e = sk.store_put(up)
        up = e.get()
    assert _put_raw(sk, up.chars)[0] == FHS_ERR_LIMIT


def test_rotation_groups_survive_parking(sk):
    """x + 1 and x + 2 in fused mode share one blind rotation per block 0 (same table, same input up to the trivial
    constant): their sum is charged as fully correlated, (1 + 1)^2 = 4, where two independent blocks cost 2 (the carry
    block's 3 is the largest other input of the addition).  The same holds for the restored blocks, also when they come
    from two separate get calls, and between a restored block and an original."""
    from fhestring_amd.api import FheString
    sk.set_mode(1)

    def add_cost(p, q):
        sk.stats(reset=True)
        r = p.add(q)
        sk.flush()
        return sk.stats()["max_input_sum_c2"]

    x, y = sk.dummy_string(2).chars
    r1, r2 = x.add(sk.trivial(1)), x.add(sk.trivial(2))
    sk.flush()
    assert sk.stats()["pbs_extracted"] >= 1                                      # the planner shares rotations
    assert add_cost(x, y) == 3 and add_cost(r1, r2) == 4
    e = sk.store_put(FheString([r1, r2, y]))
    both = e.get()
    assert add_cost(both[0], both[1]) == 4
    first, second = e.get(0, 1)[0], e.get(1, 1)[0]
    assert add_cost(first, second) == 4 and add_cost(first, r2) == 4
    assert add_cost(both[0], both[2]) == 3 and add_cost(first, y) == 3
    # import draws fresh groups, once per entry: blocks of one imported entry stay correlated, two imports of the same
    # bytes are strangers to each other
    from fhestring_amd.api import CompactFheString, store_meta_word
    c = CompactFheString(2, np.zeros((1, N), np.uint32), np.zeros(8, np.uint32))
    meta = np.array([store_meta_word(1, 1, 7 if t % 4 == 0 else 0) for t in range(8)], np.uint64)
    i1, i2 = sk.store_import(c, meta), sk.store_import(c, meta)
    p, q = i1.get().chars
    assert add_cost(p, q) == 4 and add_cost(p, i2.get(1, 1)[0]) == 3 and add_cost(p, first) == 3
    assert add_cost(*sk.store_import(c).get().chars) == 3                        # meta=None: fresh uploads, no group


def test_entries(sk):
    s = sk.dummy_string(4097)
    ids = []
    for n in (1, 512, 513, 4097):
        e = sk.store_put(s.chars[:n])
        ids.append(e.id)
        assert len(e) == n and e.device_bytes == 8192 * ((4 * n + N - 1) // N) + 16 * n
    assert e.device_bytes == 139280
    assert 0 not in ids and len(set(ids)) == 4
    st = sk.store_stats()
    assert st == {"entries": 4, "chars": 1 + 512 + 513 + 4097, "device_bytes": 8208 + 16384 + 24592 + 139280}
    L, h = sk.ctx._L, sk.ctx._h
    hs = (C.c_uint64 * 8)()
    assert L.fhs_store_get(h, e.id, 4097, 1, hs) == FHS_ERR_ARG                  # windows outside the entry
    assert L.fhs_store_get(h, e.id, 4090, 8, hs) == FHS_ERR_ARG
    assert L.fhs_store_get(h, e.id, 4098, 0, hs) == FHS_ERR_ARG
    assert L.fhs_store_get(h, e.id, 4089, 8, hs) == 0
    for k in range(8):
        assert L.fhs_release(h, hs[k]) == 0
    assert L.fhs_store_get(h, 12345, 0, 1, hs) == FHS_ERR_ARG                    # unknown id
    assert L.fhs_store_info(h, 12345, None, None) == FHS_ERR_ARG and L.fhs_store_drop(h, 12345) == FHS_ERR_ARG
    assert L.fhs_store_drop(h, 0) == FHS_ERR_ARG
    assert _put_raw(sk, []) == (FHS_ERR_ARG, 0)                                  # no characters: no entry, no id
    e.drop()
    assert sk.store_stats() == {"entries": 3, "chars": 1026, "device_bytes": 8208 + 16384 + 24592}
    assert L.fhs_store_drop(h, e.id) == FHS_ERR_ARG and L.fhs_store_get(h, e.id, 0, 1, hs) == FHS_ERR_ARG
    again = sk.store_put(s.chars[:1])
    assert again.id not in ids                                                   # ids are never reused
    from fhestring_amd.api import FhsError
    with pytest.raises(FhsError) as err:
        again.export()                                                           # a planner holds no ciphertext
    assert err.value.code == FHS_ERR_STATE


def test_export_bytes_and_import_checks(ck, sk):
    from fhestring_amd.api import (CompactFheString, FhsError, pack_host, pack_switch32, store_export_from_bytes,
                                   store_export_to_bytes, store_meta_word)
    c = pack_switch32(*pack_host(ck.packing_key(), ck.encrypt_str_raw("disk", 1)), 20)
    meta = np.array([store_meta_word(1 + t, t % 17, t // 4) for t in range(20)], np.uint64)
    assert int(meta[5]) == 6 | 5 << 16 | 1 << 32
    data = store_export_to_bytes(c, meta)
    assert len(data) == len(c.to_bytes()) + 16 + 8 * 20 and data[len(c.to_bytes()):][:8] == b"FHSSMET1"
    c2, meta2 = store_export_from_bytes(data)
    assert c2.to_bytes() == c.to_bytes() and np.array_equal(meta2, meta)
    for bad in (data[:-8], data + b"\0" * 8, c.to_bytes(), data.replace(b"FHSSMET1", b"FHSSMET2"), b""):
        with pytest.raises(ValueError):
            store_export_from_bytes(bad)
    e = sk.store_import(c2, meta2)
    assert len(e) == 5 and e.device_bytes == 8192 + 80
    assert [h.sum_c2() for h in e.get().chars] == [4, 8, 12, 16, 20]             # the largest figure of each character
    assert len(sk.store_import(c)) == 5                                          # meta=None
    for t, word in ((0, store_meta_word(0, 1)), (19, store_meta_word(3, 17)), (7, store_meta_word(1, 0) | np.uint64(1 << 24))):
        bad = meta.copy()
        bad[t] = word
        with pytest.raises(FhsError) as err:
            sk.store_import(c, bad)
        assert err.value.code == FHS_ERR_ARG
    assert sk.store_stats()["entries"] == 2
    # cycles travel: an entry imported at 16 comes back at 16 and cannot be parked again before a bootstrap
    e16 = sk.store_import(c, np.full(20, store_meta_word(1, 16), np.uint64))
    assert _put_raw(sk, e16.get().chars)[0] == FHS_ERR_LIMIT
    e15 = sk.store_import(c, np.full(20, store_meta_word(1, 15), np.uint64))
    assert _put_raw(sk, e15.get().chars)[0] == 0
