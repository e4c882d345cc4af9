"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/fhestring_hip.h declares, fails loudly without a GPU, and the host-side client works."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "fhestring_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fhs_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import fhestring_amd
    L = ctypes.CDLL(fhestring_amd.LIB_PATH)
    names = _declared()
    assert len(names) >= 70
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def _header_functions():
    """{name: number of parameters} straight from the header's text (not through fhestring_amd.cabi)"""
    text = open(os.path.join(ROOT, "include", "fhestring_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"typedef[^;{]*\([^;]*;", "", text)                     # the callback typedef is no function
    return {name: 0 if params.strip() == "void" else params.count(",") + 1
            for name, params in re.findall(r"\b(fhs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}


def test_every_header_function_has_a_derived_prototype():
    """_lib._declare is a loop over the header: every function is declared, with the header's arity; a handful of
    prototypes are pinned as literals so that a change of the derivation rule shows."""
    import ctypes as C
    import fhestring_amd
    L = fhestring_amd.lib()
    want = _header_functions()
    assert sorted(want) == _declared() and len(want) >= 186
    for name, arity in want.items():
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == arity, name
    vp, u64, sz, i = C.c_void_p, C.c_uint64, C.c_size_t, C.c_int
    assert (L.fhs_eq.restype, L.fhs_eq.argtypes) == (u64, [vp, u64, u64])
    assert (L.fhs_ctx_create.restype, L.fhs_ctx_create.argtypes) == (i, [i, vp])
    assert (L.fhs_client_decrypt_str.restype, L.fhs_client_decrypt_str.argtypes) == (i, [vp, vp, sz, C.c_char_p, vp])
    assert (L.fhs_last_error.restype, L.fhs_last_error.argtypes) == (C.c_char_p, [vp])
    assert (L.fhs_client_bsk.restype, L.fhs_client_bsk.argtypes) == (C.POINTER(u64), [vp])
    assert (L.fhs_store_get.restype, L.fhs_store_get.argtypes) == (i, [vp, u64, sz, sz, vp])


def test_structs_are_the_headers():
    import ctypes as C
    from fhestring_amd._lib import CaptureRec, Stats
    assert C.sizeof(Stats) == 64 and C.sizeof(CaptureRec) == 32
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fhestring_hip.h")).read(), flags=re.S)
    for cls, name in ((Stats, "fhs_stats"), (CaptureRec, "fhs_capture_rec")):
        body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % name, text).group(1)
        fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert [f for f, _ in cls._fields_] == fields, name
    assert [f for f, _ in Stats._fields_][0] == "pbs_executed" and [f for f, _ in CaptureRec._fields_][-1] == "width"
    assert dict(CaptureRec._fields_)["sum_c2"] is C.c_int64 and dict(CaptureRec._fields_)["konst"] is C.c_int32


def test_void_pointer_parameters_take_what_the_wrappers_pass_and_nothing_looser():
    """Pointer parameters are c_void_p: it accepts every kind of object the wrappers hand over, and still rejects a bare
    ndarray, so a wrapper that forgets _ptr() fails loudly instead of passing garbage."""
    import ctypes as C
    a = np.zeros(4, np.uint64)
    word = C.c_uint64()
    for ok in ((C.c_uint64 * 4)(), C.byref(word), a.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.POINTER(C.c_uint64)),
               a.ctypes.data_as(C.POINTER(C.c_double)), C.create_string_buffer(16), b"bytes", None, a.ctypes.data,
               C.c_char_p(b"x")):
        C.c_void_p.from_param(ok)
    for bad in (a, 1.5, [1, 2]):
        with pytest.raises(TypeError):
            C.c_void_p.from_param(bad)
    import fhestring_amd
    with pytest.raises(C.ArgumentError):                    # refused while converting: the function is never entered
        fhestring_amd.lib().fhs_fft_mono_table(np.zeros(8192))


def test_no_gpu_fails_loudly_not_silently():
    import torch
    import fhestring_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(fhestring_amd.FhsError, match="no CPU fallback"):
        fhestring_amd.Context(0)


def _run_py(code, **env):
    import subprocess
    import sys
    e = dict(os.environ, **env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def test_loader_keeps_one_hip_runtime_in_the_process():
    """Round 2's call_b.log segmentation faults: the library loaded before torch leaves /opt/rocm's HIP runtime in the
    process, a later `import torch` maps PyTorch's own copy beside it (different RPATH), and the first GPU call of
    either side crashes.  lib() now imports torch first (one shared runtime), and refuses to go on when two runtimes
    are mapped."""
    # default order: fhestring_amd first, torch afterwards -> still ONE runtime, no error
    p = _run_py("import fhestring_amd, torch\n"
                "from fhestring_amd._lib import hip_runtimes, check_single_hip_runtime\n"
                "fhestring_amd.lib(); check_single_hip_runtime(); print(len(hip_runtimes()))")
    assert p.returncode == 0, p.stderr[-800:]
    assert p.stdout.strip().endswith("1"), p.stdout
    # the old behaviour (preload switched off), then torch: two runtimes -> FhsError instead of a crash
    p = _run_py("import fhestring_amd\n"
                "fhestring_amd.lib()\n"
                "import torch\n"
                "from fhestring_amd._lib import hip_runtimes\n"
                "print(len(hip_runtimes()))\n"
                "try:\n"
                "    fhestring_amd.Context(0)\n"
                "except fhestring_amd.FhsError as e:\n"
                "    print('FhsError:', e)\n", FHS_SKIP_TORCH_PRELOAD="1")
    assert p.returncode == 0, p.stderr[-800:]
    assert "2\nFhsError: two HIP runtimes" in p.stdout, p.stdout


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "fhestring_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("oracle/radix.py", "").replace("oracle/strings.py", "") \
                    .replace("the oracle", "").replace("oracle's", "").replace("CPU oracle", ""), (dp, f)


def test_client_roundtrip_and_cross_decrypt_with_oracle():
    """The product's client (host CPU, like the reference's) against the oracle's decrypt."""
    from fhestring_amd.api import MyClientKey
    from oracle import core
    ck = MyClientKey(1234)
    try:
        lwe, glwe = ck.secret_keys()
        assert set(np.unique(lwe)) <= {0, 1} and set(np.unique(glwe)) <= {0, 1}
        assert not np.any(ck.bsk() & np.uint64(63))          # 58-bit torus grid
        for v in (0, 1, 0x41, 0xFF):
            ct = ck.encrypt_char_raw(v)
            assert ck.decrypt_char_raw(ct) == v
            blocks = [int(core.lib().orc_decrypt_block(glwe, np.ascontiguousarray(ct[i]))) for i in range(4)]
            assert blocks == [(v >> (2 * i)) & 3 for i in range(4)]
        s = ck.encrypt_str_raw("hello world", 3)
        assert s.shape == (14, 4, 2049)
        assert ck.decrypt_str_raw(s) == "hello world"          # truncates at the first NUL
        with pytest.raises(AssertionError):
            ck.encrypt_str_raw("bad\0string", 1)               # client_key.rs:52-55
    finally:
        ck.close()


def test_string_encryption_is_threaded_and_independent_of_the_thread_count():
    """fhs_client_encrypt_str / _decrypt_str share one string's characters among host threads (config 5 hands over 2 x
    4097 characters = 537 MB): every character draws from its own (mask, noise) ChaCha20 streams keyed by call number and
    index, so the ciphertexts do not depend on the number of threads; a second call never reuses a stream; the result
    decrypts under the oracle's arithmetic too."""
    import os
    from fhestring_amd.api import MyClientKey
    from oracle import core
    text = "".join(chr(0x20 + (7 * i) % 95) for i in range(300))
    old = os.environ.get("FHS_CLIENT_THREADS")
    try:
        os.environ["FHS_CLIENT_THREADS"] = "1"
        a = MyClientKey(1234)
        x1 = a.encrypt_str_raw(text, 1)
        os.environ["FHS_CLIENT_THREADS"] = "6"
        b = MyClientKey(1234)
        x6 = b.encrypt_str_raw(text, 1)
        assert x1.shape == (301, 4, 2049) and np.array_equal(x1, x6)
        y6 = b.encrypt_str_raw(text, 1)
        assert not np.array_equal(y6[:, :, :8], x6[:, :, :8])                     # fresh masks on every call
        assert len({bytes(x6[i, k, :4]) for i in range(301) for k in range(4)}) == 1204   # no two blocks share a mask stream
        assert b.decrypt_str_raw(y6) == text and a.decrypt_str_raw(x6) == text
        _, glwe = a.secret_keys()
        got = [sum(int(core.lib().orc_decrypt_block(glwe, np.ascontiguousarray(x1[i, k]))) << (2 * k) for k in range(4))
               for i in (0, 17, 299, 300)]
        assert got == [ord(text[0]), ord(text[17]), ord(text[299]), 0]
        a.close(); b.close()
    finally:
        if old is None:
            os.environ.pop("FHS_CLIENT_THREADS", None)
        else:
            os.environ["FHS_CLIENT_THREADS"] = old


def test_product_keys_bootstrap_correctly_under_the_oracle():
    """Keys generated by the product's client are valid: the oracle PBS decrypts f(m) with them."""
    from fhestring_amd.api import MyClientKey
    from oracle import core, radix
    ck = MyClientKey(77)
    try:
        _, glwe = ck.secret_keys()
        S = core.ServerKey(ck.bsk().copy(), ck.ksk().copy())
        ch = ck.encrypt_char_raw(0b11100100)                   # blocks 0,1,2,3
        outs = S.pbs_batch(ch, np.zeros(4, np.uint32), radix.lut_poly("carry")[None] * 0 + radix.lut_poly("msg")[None])
        assert [int(core.lib().orc_decrypt_block(glwe, np.ascontiguousarray(o))) for o in outs] == [0, 1, 2, 3]
    finally:
        ck.close()


def test_key_file_roundtrip(tmp_path):
    """raw little-endian key files (client key and server-key-only)."""
    from fhestring_amd.api import MyClientKey
    import fhestring_amd
    ck = MyClientKey(99)
    try:
        full, pub = tmp_path / "client.key", tmp_path / "server.key"
        ck.save(full)
        ck.save(pub, server_key_only=True)
        assert pub.stat().st_size == 64 + (742 * 4 * 2048 + 2048 * 5 * 743) * 8
        assert full.stat().st_size == pub.stat().st_size + 8 + (742 + 2048) * 8
        ck2 = MyClientKey.load(full)
        try:
            assert np.array_equal(ck2.bsk(), ck.bsk()) and np.array_equal(ck2.ksk(), ck.ksk())
            assert all(np.array_equal(a, b) for a, b in zip(ck2.secret_keys(), ck.secret_keys()))
            ct = ck.encrypt_str_raw("key file", 1)
            assert ck2.decrypt_str_raw(ct) == "key file"
        finally:
            ck2.close()
        with pytest.raises(fhestring_amd.FhsError):
            MyClientKey.load(pub)                 # a server-key file holds no secret key
        pair = tmp_path / "pair.key"              # kind 3: the pair key of the two-key-bits-per-product arithmetics
        ck.save_multibit_key(pair)
        assert pair.stat().st_size == 64 + 371 * 3 * 4 * 2048 * 8
        raw = np.fromfile(pair, dtype=np.uint64, offset=64)
        assert np.array_equal(raw, ck.bsk_mb2()) and pair.read_bytes()[:8] == b"FHSKEY01"
        with pytest.raises(fhestring_amd.FhsError):
            MyClientKey.load(pair)                # ... is neither a client key
        bad = tmp_path / "bad.key"
        bad.write_bytes(full.read_bytes()[:1000])
        with pytest.raises(fhestring_amd.FhsError):
            MyClientKey.load(bad)
    finally:
        ck.close()


def test_fft_twiddle_tables_match_the_oracle_on_this_host():
    """Product host code (C++ std::cos/sin) and oracle (C cos/sin) must derive bit-identical twiddles: the GPU
    FFT-mode parity test compares outputs bit for bit and starts from these tables (no GPU needed here)."""
    import numpy as np
    from fhestring_amd._lib import fft_tables
    from oracle import core
    got, want = fft_tables(), core.fft_tables()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert abs(got[0][1] - np.cos(np.pi / 4)) < 1e-15


def test_monomial_table_of_the_two_bit_kernel_matches_the_oracle_on_this_host():
    """exp(i pi k / 2048), k < 4096, of FHS_ARITH_F64_FFT_MB2: product host code and oracle call cos() / sin() through
    volatile pointers -- a fused sincos() differs in the last place for a few arguments (seen: 2 of 8192 entries)."""
    import ctypes as C
    import numpy as np
    from fhestring_amd._lib import lib
    from oracle import core
    got, want = np.zeros(8192), np.zeros(8192)
    L = lib()
    L.fhs_fft_mono_table(got.ctypes.data_as(C.c_void_p))
    O = core.lib()
    O.orc_fft_mono_table.argtypes = [C.c_void_p]
    O.orc_fft_mono_table.restype = None
    O.orc_fft_mono_table(want.ctypes.data_as(C.c_void_p))
    assert np.array_equal(got, want)
    assert got[0] == 1.0 and got[1] == 0.0 and abs(got[2 * 1024 + 1] - 1.0) < 1e-15


def test_client_pair_key_encrypts_the_products_of_key_bits():
    """fhs_client_bsk_mb2: for every pair (s, s') of LWE key bits the GGSWs of s(1-s'), (1-s)s', s s'.  Checked with the
    client's own secret keys: row 1 of each GGSW is a GLWE encryption of msg * 2^41 (constant coefficient), on the
    58-bit grid, and the product's pair key works under the oracle's mode 4 bootstrap."""
    import numpy as np
    from fhestring_amd.api import MyClientKey
    from oracle import core, radix
    ck = MyClientKey(78)
    try:
        lwe, glwe = ck.secret_keys()
        mb = ck.bsk_mb2().reshape(371, 3, 2, 2, 2048)
        assert not (mb & np.uint64(63)).any()
        for p in (0, 1, 17, 370):
            s1, s2 = int(lwe[2 * p]), int(lwe[2 * p + 1])
            want = [s1 * (1 - s2), (1 - s1) * s2, s1 * s2]
            for t in range(3):
                mask, body = mb[p, t, 1, 0], mb[p, t, 1, 1]
                # constant coefficient of mask (*) S:  a[0] S[0] - sum_{j>=1} a[N-j] S[j]
                dot = int(mask[0]) * int(glwe[0]) - sum(int(a) * int(s) for a, s in zip(mask[:0:-1], glwe[1:]))
                phase = (int(body[0]) - dot) & (2**64 - 1)
                assert ((phase + (1 << 40)) >> 41) & ((1 << 23) - 1) == want[t], (p, t)
        S = core.ServerKey(ck.bsk().copy(), ck.ksk().copy()).set_mb2(mb)
        ch = ck.encrypt_char_raw(0b11100100)
        outs = S.pbs_batch(ch, np.zeros(4, np.uint32), radix.lut_poly("msg")[None], mode=4)
        assert [int(core.lib().orc_decrypt_block(glwe, np.ascontiguousarray(o))) for o in outs] == [0, 1, 2, 3]
    finally:
        ck.close()


def test_client_generator_is_chacha20_and_os_seeded_by_default():
    """keys, masks and noise come from ChaCha20 keyed with OS entropy; the 64-bit-seed path is an
    explicitly insecure test constructor.  RFC 8439 section 2.3.2 known-answer test for the block function."""
    import ctypes as C
    import fhestring_amd
    from fhestring_amd.api import MyClientKey
    L = fhestring_amd.lib()
    key = (C.c_uint32 * 8)(*[int.from_bytes(bytes(range(4 * i, 4 * i + 4)), "little") for i in range(8)])
    nonce = (C.c_uint32 * 3)(0x09000000, 0x4A000000, 0x00000000)
    out = (C.c_uint32 * 16)()
    L.fhs_chacha20_block(key, 1, nonce, out)
    assert list(out) == [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
                         0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]
    # the generator draws eight blocks at a time (AVX2): same keystream as a plain RFC 8439 block function, also across
    # the 32-bit counter's wrap (scalar path there)
    def block(key, counter, nonce):
        st = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + list(key) + [counter] + list(nonce)
        x = st[:]
        rot = lambda v, n: ((v << n) | (v >> (32 - n))) & 0xFFFFFFFF
        def qr(a, b, c, d):
            x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rot(x[d] ^ x[a], 16)
            x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rot(x[b] ^ x[c], 12)
            x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rot(x[d] ^ x[a], 8)
            x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rot(x[b] ^ x[c], 7)
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        return [(x[i] + st[i]) & 0xFFFFFFFF for i in range(16)]
    assert block(list(key), 1, list(nonce)) == list(out)
    for start in (1, 0xFFFFFFE0):
        n_blocks = 40
        draws = (C.c_uint64 * (8 * n_blocks))()
        L.fhs_chacha20_stream(key, start, nonce, draws, 8 * n_blocks)
        want = []
        ctr, nn = start, list(nonce)
        for _ in range(n_blocks):
            w = block(list(key), ctr, nn)
            want += [w[2 * i] | (w[2 * i + 1] << 32) for i in range(8)]
            ctr = (ctr + 1) & 0xFFFFFFFF
            if ctr == 0:
                nn[0] = (nn[0] + 0x100) & 0xFFFFFFFF  # the generator's own carry rule (above the domain byte)
        assert list(draws) == want, hex(start)
    a, b = MyClientKey(), MyClientKey()               # OS entropy: two clients never share keys
    s1, s2 = MyClientKey(5), MyClientKey(5)           # insecure seeded: reproducible
    try:
        assert not np.array_equal(a.secret_keys()[1], b.secret_keys()[1])
        assert not np.array_equal(a.encrypt_char_raw(65), b.encrypt_char_raw(65))
        assert a.decrypt_char_raw(a.encrypt_char_raw(0xA5)) == 0xA5
        assert np.array_equal(s1.secret_keys()[0], s2.secret_keys()[0]) and np.array_equal(s1.ksk(), s2.ksk())
        assert np.array_equal(s1.encrypt_char_raw(65), s2.encrypt_char_raw(65))
        # masks are uniform u64 and the secret key is balanced binary
        lwe, glwe = a.secret_keys()
        assert 900 < int(glwe.sum()) < 1150 and 300 < int(lwe.sum()) < 440
    finally:
        for k in (a, b, s1, s2):
            k.close()


def test_c_host_builds_as_c99_and_fails_loudly_without_a_gpu():
    """examples/c_host.c: a compiled host over the C ABI in plain C99 (what a Rust binding of the reference would be,
    minus the language) -- the header compiles as C with -pedantic -Werror, the program links against the in-tree
    library alone, and where no MI355X is visible it says so and exits non-zero instead of falling back to anything."""
    import subprocess
    exe = os.path.join(ROOT, "examples", "c_host")
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run([exe, "hello world", "wor"], capture_output=True, text=True, timeout=300)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        assert out.returncode == 0, out.stdout + out.stderr
    else:
        assert out.returncode == 2 and "no CPU fallback" in out.stderr and "Test Passed" not in out.stdout


def test_device_pointer_entries_refuse_on_the_host():
    """fhs_export_device(_async), fhs_import_device and fhs_stream_handle where the library answers before it touches a
    GPU: a planner context computes nothing and exports nothing; null pointers and released handles are argument errors.
    (What the entries do with valid device pointers is tests/test_gpu_device_boundary.py.)"""
    import ctypes as C
    from fhestring_amd.api import MyServerKey
    FHS_ERR_ARG, FHS_ERR_STATE = -1, -3
    sk = MyServerKey.planner()
    try:
        L, h = sk.ctx._L, sk.ctx._h
        last = lambda: L.fhs_last_error(h).decode()
        room = np.zeros(4 * 2049, np.uint64)                  # a valid destination, should an entry ever write
        dst = room.ctypes.data_as(C.c_void_p)
        t = sk.trivial(0x41)
        for entry in (L.fhs_export_device, L.fhs_export_device_async):
            assert entry(h, t.h, dst) == FHS_ERR_STATE and "planner context" in last()
            assert entry(h, t.h, None) == FHS_ERR_ARG and "null argument" in last()
            assert entry(h, 0, dst) == FHS_ERR_ARG
            assert entry(None, t.h, dst) == FHS_ERR_ARG
        assert not room.any()
        gone = sk.trivial(0x42)
        released, gone.h = gone.h, 0                          # (the Python object must not release it a second time)
        assert L.fhs_release(h, released) == 0
        for entry in (L.fhs_export_device, L.fhs_export_device_async):
            assert entry(h, released, dst) == FHS_ERR_ARG and "invalid handle" in last()
        assert L.fhs_import_device(h, None) == 0 and "null argument" in last()
        assert L.fhs_import_device(None, dst) == 0
        assert L.fhs_stream_handle(None) is None
        assert L.fhs_stream_handle(h) is None                 # a planner has no stream
    finally:
        sk.close()


def test_import_device_on_a_planner_context_books_a_block_and_copies_nothing():
    """Pinned as it is today: on a planner fhs_import_device is an upload for the bookkeeping -- four fresh blocks at
    figure 1, usable as operands -- and the source is never read."""
    import ctypes as C
    from fhestring_amd import FhsError
    from fhestring_amd.api import FheAsciiChar, MyServerKey
    from test_gpu_packed import _kinds                        # block kinds through fhs_debug_char_terms; needs no GPU
    sk = MyServerKey.planner()
    try:
        src = np.full(4 * 2049, 0xA5A5A5A5A5A5A5A5, np.uint64)
        before = sk.stats()["blocks_live"]
        ch = FheAsciiChar(sk, sk.ctx._L.fhs_import_device(sk.ctx._h, src.ctypes.data_as(C.c_void_p)))
        assert sk.stats()["blocks_live"] == before + 4
        assert ch.sum_c2() == 1 and _kinds(sk, ch) == [1] * 4 and ch.trivial_value() is None
        assert ch.set_noise(3).sum_c2() == 3
        with pytest.raises(FhsError) as e:
            ch.set_noise(0)
        assert e.value.code == -1 and ch.sum_c2() == 3
        sk.set_mode(0)
        r = ch.bitand(sk.upload_char(np.zeros((4, 2049), np.uint64)))
        sk.flush()
        assert sk.stats()["pbs_executed"] == 4 and r.sum_c2() == 1
        with pytest.raises(FhsError, match="planner context") as e:
            ch.download()
        assert e.value.code == -3
        assert (src == 0xA5A5A5A5A5A5A5A5).all()
    finally:
        sk.close()
