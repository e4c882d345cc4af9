"""The device-pointer boundary of include/fhestring_hip.h on the MI355X: fhs_import_device, fhs_export_device,
fhs_export_device_async, fhs_stream_handle and fhs_pbs_batch_device on a caller's stream -- the entry points through
which another GPU program (torch, RCCL) hands ciphertexts in and takes them out without touching the host.

Every export lands in the middle of a tensor filled with a sentinel: the guard words on both sides must survive, so a
wrong stride or offset of the packed [4][2049] caller layout against the pool's rows shows.  Device buffers are
torch.int64 tensors read back as uint64.  Every device pointer handed to the library is valid and large enough; argument
errors are in tests/test_cabi.py, where the library refuses on the host.  Two contexts for the module (f64 FFT and exact
NTT, the session's oracle keys); loops instead of parametrisation (the GPU suite's item count is capped in conftest.py)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_packed import _kinds
from test_gpu_wide_parity import _oracle_bitand

pytestmark = pytest.mark.gpu

BIG_CT = 2049
BIG_N = 2048
W = 4 * BIG_CT                                   # words of one character in the caller's layout
PAD = 64                                         # guard words on each side of an export
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
FHS_ERR_ARG = -1
NAMES = ["msg", "carry", "eq_biv", "sign", "cmp_le"]


@pytest.fixture(scope="module")
def sk_fft(oracle_keys):
    import fhestring_amd
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.from_raw_keys(oracle_keys.bsk, oracle_keys.ksk, arith=fhestring_amd.Context.ARITH_F64_FFT)
    sk.set_mode(1)
    yield sk
    sk.close()


@pytest.fixture(scope="module")
def sk_exact(oracle_keys):
    import fhestring_amd
    from fhestring_amd.api import MyServerKey
    sk = MyServerKey.from_raw_keys(oracle_keys.bsk, oracle_keys.ksk, arith=fhestring_amd.Context.ARITH_EXACT_NTT)
    sk.set_mode(1)
    yield sk
    sk.close()


class Landing:
    """A device tensor of PAD + shift + n_chars * W + PAD sentinel words; exports go to word PAD + shift.  shift = 1 makes
    the destination 8-byte but not 16-byte aligned (torch's allocations start on 512 bytes, PAD words are 512 bytes)."""

    def __init__(self, n_chars=1, shift=0):
        import torch
        self.n, self.at = n_chars, PAD + shift
        self.t = torch.full((self.at + n_chars * W + PAD,), int(SENTINEL) - (1 << 64), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()                 # the fill ran on torch's stream, the library's stream does not wait for it
        assert self.ptr() % 16 == (8 if shift % 2 else 0)

    def ptr(self, i=0):
        return self.t.data_ptr() + 8 * (self.at + i * W)

    def words(self, what):
        """After the caller's wait: the guards are intact -> [n_chars][4][2049] words of the region."""
        host = self.t.cpu().numpy().view(np.uint64)
        end = self.at + self.n * W
        assert (host[:self.at] == SENTINEL).all(), ("words in front of the destination were overwritten", what)
        assert (host[end:] == SENTINEL).all() and host[end:].size == PAD, ("words behind the destination were overwritten", what)
        return host[self.at:end].reshape(self.n, 4, BIG_CT).copy()


def _export(sk, ch, what, shift=0):
    """fhs_export_device itself, not api.export_device (which flushes first and so hides the entry's own flush)."""
    import torch
    land = Landing(1, shift)
    sk.ctx._check(sk.ctx._L.fhs_export_device(sk.ctx._h, ch.h, C.c_void_p(land.ptr())))
    torch.cuda.synchronize()
    return land.words(what)[0]


def _dev(a):
    """host array -> device tensor of the same bytes, complete before the library's stream may read it"""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])).cuda()
    torch.cuda.synchronize()
    return t


def test_export_of_every_block_kind(sk_fft, sk_exact, oracle_keys, oracle_sk):
    """fhs_export_device of an uploaded character (MAT), a trivial one (TRIV: a 16 392-byte memset plus one 32-bit memset
    on the high half of the body word), a result whose bootstraps are still pending (the entry's own flush; against the
    oracle in both arithmetics) and a pending sum (LIN: materialised on the way out, keeps its noise figure)."""
    sk, keys = sk_fft, oracle_keys
    # uploaded characters, at a 16-byte and at an 8-byte aligned destination
    for v in (0x00, 0x5A, 0xFF):
        words = keys.encrypt_char(v)
        ch = sk.upload_char(words)
        for shift in (0, 1):
            assert np.array_equal(_export(sk, ch, ("uploaded", hex(v), shift), shift), words), ("uploaded", hex(v), "shift", shift)
    # trivial characters: every mask word 0, body = two message bits << 59
    for v in (0x00, 0x1B, 0xFF):
        ch = sk.trivial(v)
        got = _export(sk, ch, ("trivial", hex(v)))
        assert not (got == SENTINEL).any(), ("trivial: sentinel left inside the destination", hex(v))
        assert not got[:, :BIG_N].any(), ("trivial: non-zero mask word", hex(v))
        assert [int(b) for b in got[:, BIG_N]] == [((v >> (2 * i)) & 3) << 59 for i in range(4)], ("trivial body", hex(v))
        if v == 0xFF:
            assert [int(b) for b in got[:, BIG_N]] == [0x1800000000000000] * 4
        assert _kinds(sk, ch) == [0] * 4, ("trivial stays plaintext after the export", hex(v))
    # pending bootstraps: as-written bitand, not flushed; the export flushes, copies behind the kernels and waits
    va, vb = 0xC5, 0x6E
    a_ct, b_ct = keys.encrypt_char(va), keys.encrypt_char(vb)
    for s, mode, name in ((sk_fft, 3, "f64 fft"), (sk_exact, 0, "exact")):
        s.set_mode(0)
        try:
            r = s.upload_char(a_ct).bitand(s.upload_char(b_ct))
            s.stats(reset=True)
            assert s.stats()["pbs_executed"] == 0
            got = _export(s, r, ("pending bitand", name))
            assert s.stats()["pbs_executed"] == 4, ("the export's own flush ran the four bootstraps", name)
        finally:
            s.set_mode(1)
        assert np.array_equal(got, _oracle_bitand(oracle_sk, a_ct, b_ct, mode)), ("pending bitand differs from the oracle", name)
        assert keys.decrypt_char(got) == va & vb, name
    # pending sums, both outcomes of the condition; _kinds flushes (fhs_debug_char_terms), so in the third case nothing looks
    # at the handle first and the sum's own bootstraps are still pending when the export is called
    for v0, v1, look in ((0x33, 0x33, True), (0x33, 0x34, True), (0x35, 0x35, False)):
        c = [sk.upload_char(keys.encrypt_char(v)) for v in (v0, v1, 0x7E, 0x81)]
        x = c[0].eq(c[1]).if_then_else(c[2], c[3])
        sk.stats(reset=True)
        assert x.sum_c2() == 2 and sk.stats()["pbs_executed"] == 0, (v0, v1)
        if look:
            assert _kinds(sk, x) == [2] * 4, ("a pending sum per block before the export", v0, v1)
        ran = sk.stats()["pbs_executed"]
        assert (ran > 0) == look, (v0, v1)
        got = _export(sk, x, ("pending sum", v0, v1))
        assert look or sk.stats()["pbs_executed"] > ran, ("the export's own flush ran the sum's bootstraps", v0, v1)
        assert _kinds(sk, x) == [1] * 4, ("materialised by the export", v0, v1)
        assert x.sum_c2() == 2, ("the materialised sum keeps its figure", v0, v1)
        assert np.array_equal(got, x.download()), ("export differs from the download of the same handle", v0, v1)
        assert keys.decrypt_char(got) == (0x7E if v0 == v1 else 0x81), (v0, v1)


def test_import_equals_upload(sk_fft, oracle_keys):
    """fhs_import_device: the imported handle holds the source's words, enters the ledger at figure 1 as a block, and
    computes like an uploaded twin bit for bit; the source may be overwritten once the context's stream has passed the
    copy (the contract stated at fhs_import_device in the header)."""
    import torch
    from fhestring_amd import FhsError
    from fhestring_amd.api import FheString
    sk, keys = sk_fft, oracle_keys
    vals = [0x00, 0xFF, 0x61, 0x61, 0x5A, 0x7B]
    words = np.stack([keys.encrypt_char(v) for v in vals])                    # [6][4][2049]
    src = _dev(words)
    imp = [sk.import_device(src[i].data_ptr()) for i in range(6)]
    for i, h in enumerate(imp):
        assert np.array_equal(h.download(), words[i]), ("imported words", i)
        assert h.sum_c2() == 1 and _kinds(sk, h) == [1] * 4, ("imported block kind / figure", i)
    try:
        for mode in (0, 1):
            sk.set_mode(mode)
            up = [sk.upload_char(words[i]) for i in range(6)]
            res = []
            for c in (imp, up):
                res.append([c[2].eq(c[3]), c[0].eq(c[1]), c[1].bitand(c[4]), c[2].bitand(c[5])] + sk.to_upper(FheString(c)).chars)
            got_i, got_u = ([r.download() for r in rs] for rs in res)
            for k, (x, y) in enumerate(zip(got_i, got_u)):
                assert np.array_equal(x, y), ("imported and uploaded operands give different words", "mode", mode, "result", k)
            want = [1, 0, 0xFF & 0x5A, 0x61 & 0x7B] + list(bytes(vals).upper())
            assert [keys.decrypt_char(x) for x in got_i] == want, ("mode", mode)
    finally:
        sk.set_mode(1)
    # source lifetime: once the context's stream has passed the copy, the source is the caller's again
    t = src[4].clone()
    torch.cuda.synchronize()
    h = sk.import_device(t.data_ptr())
    sk.stream_sync()
    t.zero_()
    torch.cuda.synchronize()
    assert np.array_equal(h.download(), words[4]), "the import still read its source after fhs_stream_sync"
    # a source at an 8-byte (not 16-byte) aligned address
    big = torch.zeros(1 + W, dtype=torch.int64, device="cuda")
    big[1:] = src[1].reshape(-1)
    torch.cuda.synchronize()
    assert (big.data_ptr() + 8) % 16 == 8
    h8 = sk.import_device(big.data_ptr() + 8)
    assert np.array_equal(h8.download(), words[1]), "import from an 8-byte aligned source"
    # the ledger: a figure can be declared upwards, never downwards
    assert h.set_noise(3).sum_c2() == 3
    with pytest.raises(FhsError) as e:
        h.set_noise(0)
    assert e.value.code == FHS_ERR_ARG and h.sum_c2() == 3


def test_two_contexts_exchange_without_a_host_wait(sk_fft, sk_exact, oracle_keys):
    """fhs_export_device_async + fhs_stream_handle: context A (f64 FFT) exports unflushed results, context B (exact)
    imports them behind an event on A's stream; the first host wait of the exchange that the TEST makes is B's download.
    The first character exported is an as-written bitor: four bootstrap outputs and no sum, so its four copies are
    enqueued behind kernels that the same call has only just queued, with no wait on A's side.  A copy that is not
    ordered behind the kernels (a level is milliseconds, the copy microseconds) or an import that is not ordered behind
    the event hands B other words than A downloads afterwards.  The characters of to_upper that follow each hold one
    pending sum (block 2): the library materialises it inside the export and waits for A's stream there (materialize_lin),
    so for those the export is stream-ordered for the caller but not free of a host wait inside the library."""
    import torch
    from fhestring_amd.api import FheString
    A, B, keys = sk_fft, sk_exact, oracle_keys
    text = b"o World\0"
    n = len(text)
    va, vb = 0xA3, 0x4C
    s = A.upload_string(np.stack([keys.encrypt_char(b) for b in text]))
    land = Landing(n + 1)
    A.stats(reset=True)
    A.set_mode(0)
    try:
        plain = A.upload_char(keys.encrypt_char(va)).bitor(A.upload_char(keys.encrypt_char(vb)))   # 4 pending bootstraps
    finally:
        A.set_mode(1)
    up = A.to_upper(s)                                                        # fused mode, nothing runs yet
    chars = [plain] + up.chars
    figures = [ch.sum_c2() for ch in chars]                                   # what leaves a library carries its figure
    assert figures[0] == 1, "the as-written bitor hands back bootstrap outputs, not sums"
    assert A.stats()["pbs_executed"] == 0
    for i, ch in enumerate(chars):                                            # the first call flushes everything, unwaited
        A.export_device_async(ch, land.ptr(i))
    assert A.stats()["pbs_executed"] > 4
    ha, hb = A.stream_handle(), B.stream_handle()
    assert ha != 0 and hb != 0 and ha != hb
    sa, sb = torch.cuda.ExternalStream(ha), torch.cuda.ExternalStream(hb)
    ev = torch.cuda.Event()
    ev.record(sa)
    sb.wait_event(ev)
    got = FheString([B.import_device(land.ptr(i)).set_noise(max(1, f)) for i, f in enumerate(figures)])
    words_b = got.download()                                                  # the first host wait
    upper_b = FheString(got.chars[1:])
    hit, miss = B.contains_clear(upper_b, "WOR"), B.contains_clear(upper_b, "WOW")
    assert (keys.decrypt_char(hit.download()), keys.decrypt_char(miss.download())) == (1, 0)
    words_a = FheString(chars).download()
    assert np.array_equal(words_b[0], words_a[0]), "B imported other words than A holds (bitor, copied behind queued kernels)"
    assert np.array_equal(words_b, words_a), "B imported other words than A holds"
    assert keys.decrypt_char(words_b[0]) == va | vb
    assert bytes(keys.decrypt_char(c) for c in words_b[1:]) == text.upper()
    torch.cuda.synchronize()
    assert np.array_equal(land.words("async export of a string"), words_a)
    # A stays usable
    assert keys.decrypt_char(A.contains_clear(up, "ORL").download()) == 1
    # a torch op enqueued on A's stream right behind an async export sees the export
    va, vb = 0x3C, 0x96
    x = A.upload_char(keys.encrypt_char(va)).bitor(A.upload_char(keys.encrypt_char(vb)))      # pending
    land = Landing(1)
    with torch.cuda.stream(sa):
        A.export_device_async(x, land.ptr())
        staged = land.t.clone()
    sa.synchronize()
    staged = staged.cpu().numpy().view(np.uint64)
    want = x.download()
    assert np.array_equal(land.words("async export of a character")[0], want)
    assert np.array_equal(staged[PAD:PAD + W].reshape(4, BIG_CT), want), "the clone on the context's stream ran before the export"
    assert keys.decrypt_char(want) == va | vb


def test_pbs_batch_device_on_the_callers_stream(sk_fft, sk_exact, oracle_keys, oracle_sk):
    """fhs_pbs_batch_device enqueued on a torch stream between the caller's own copies, with no host wait from the first
    input copy to the last kernel: 7 rows (the split-K keyswitch), a clone of the result, then a wider batch into another
    output (130 rows: the wide keyswitch kernel; 33 on the exact context, whose kernel is the slow one), and on the f64
    context 300 rows more: by the sizes in Buf::reserve and ks_digits_bytes (1 MB / one group of 256 rows at least) that
    is where both scratch buffers of a fresh context have to grow while the stream may still be busy -- read from the
    code, not observed by the test.  Every word against the host path; the 7 rows against the oracle."""
    import torch
    from oracle import radix
    keys = oracle_keys
    luts = np.stack([radix.lut_poly(n) for n in NAMES])
    rng = np.random.default_rng(4)
    n_rows = 300
    msgs = rng.integers(0, 16, n_rows)
    cts = np.stack([keys.encrypt_block(int(m)) for m in msgs])
    idx = (np.arange(n_rows) % len(NAMES)).astype(np.uint32)
    h_in = torch.from_numpy(cts.view(np.int64)).pin_memory()
    h_idx = torch.from_numpy(idx.view(np.int32)).pin_memory()
    h_luts = torch.from_numpy(luts.view(np.int64)).pin_memory()
    for sk, mode, widths, name in ((sk_fft, 3, (7, 130, 300), "f64 fft"), (sk_exact, 0, (7, 33), "exact")):
        ctx = sk.ctx
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_in = h_in.to("cuda", non_blocking=True)
            d_idx = h_idx.to("cuda", non_blocking=True)
            d_luts = h_luts.to("cuda", non_blocking=True)
            outs = [torch.zeros((B, BIG_CT), dtype=torch.int64, device="cuda") for B in widths]
            ctx.pbs_batch_device(d_in.data_ptr(), d_idx.data_ptr(), d_luts.data_ptr(), outs[0].data_ptr(), widths[0],
                                 stream=s.cuda_stream)
            keep = outs[0].clone()
            for B, d_out in zip(widths[1:], outs[1:]):
                ctx.pbs_batch_device(d_in.data_ptr(), d_idx.data_ptr(), d_luts.data_ptr(), d_out.data_ptr(), B,
                                     stream=s.cuda_stream)
            s.synchronize()
        for B, d_out in zip(widths, outs):
            got = d_out.cpu().numpy().view(np.uint64)
            want = ctx.pbs_batch(cts[:B], idx[:B], luts)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, ("rows differing from the host path", name, "width", B, bad[:10])
        first = keep.cpu().numpy().view(np.uint64)
        assert np.array_equal(first, outs[0].cpu().numpy().view(np.uint64)), ("the clone behind the first call", name)
        assert np.array_equal(first, oracle_sk.pbs_batch(cts[:7], idx[:7], luts, nthreads=16, mode=mode)), ("oracle", name)
        for b in range(7):
            assert keys.decrypt_block(first[b]) == radix.lut_eval(NAMES[idx[b]], int(msgs[b])), (name, "row", b)
        # the context's own stream still works after a foreign one was used
        d_own = torch.zeros((7, BIG_CT), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.pbs_batch_device(d_in.data_ptr(), d_idx.data_ptr(), d_luts.data_ptr(), d_own.data_ptr(), 7, stream=0)
        sk.stream_sync()
        assert np.array_equal(d_own.cpu().numpy().view(np.uint64), first), ("stream 0 after a caller's stream", name)


def test_noise_figure_across_the_boundary(sk_fft, oracle_keys):
    """What leaves the library has to carry its figure: a pending sum of figure 2 is exported and imported (figure 1,
    like every import), declared with set_noise(2), and then budgets in a following add exactly like its never-exported
    twin; undeclared it would be budgeted too low.  The sum is the result of if_then_else on two flushed results: add
    itself propagates carries through bootstraps and hands back figure 1."""
    sk, keys = sk_fft, oracle_keys
    v1, v2, vf = 0x21, 0x47, 0x13
    r = sk.upload_char(keys.encrypt_char(v1)).add(sk.trivial(1))
    r2 = sk.upload_char(keys.encrypt_char(v2)).add(sk.trivial(2))
    sk.flush()
    assert r.sum_c2() == 1 and r2.sum_c2() == 1
    y, y_native = (r.eq(r2).if_then_else(r, r2) for _ in range(2))           # picks r2
    for h in (y, y_native):
        assert _kinds(sk, h) == [2] * 4 and h.sum_c2() == 2
    exported = _export(sk, y, "sum of figure 2")
    assert _kinds(sk, y) == [1] * 4 and y.sum_c2() == 2
    src = _dev(exported)
    declared, undeclared = sk.import_device(src.data_ptr()), sk.import_device(src.data_ptr())
    assert declared.sum_c2() == 1 and undeclared.sum_c2() == 1
    assert declared.set_noise(2).sum_c2() == 2
    fresh = keys.encrypt_char(vf)
    seen, results = {}, {}
    for name, h in (("native", y_native), ("declared", declared), ("undeclared", undeclared)):
        sk.stats(reset=True)
        results[name] = h.add(sk.upload_char(fresh))
        sk.flush()
        seen[name] = sk.stats()["max_input_sum_c2"]
    assert _kinds(sk, y_native) == [2] * 4                                    # the twin never left the library
    assert seen["declared"] == seen["native"], seen
    assert seen["undeclared"] < seen["native"], seen
    want = (v2 + 2 + vf) & 255
    assert [keys.decrypt_char(results[k].download()) for k in ("native", "declared", "undeclared")] == [want] * 3
