"""Thin Python mirror of the C ABI (include/fhestring_hip.h)."""
import ctypes as C

import numpy as np

from . import cabi
from ._lib import FhsError, lib, check_single_hip_runtime

_K = dict(cabi.parse_header()["consts"])      # the header's FHS_* #defines
BIG_CT = _K["FHS_BIG_CT"]
SMALL_CT = _K["FHS_SMALL_CT"]
POLY_N = _K["FHS_POLY_N"]
PACK_GROUP = _K["FHS_PACK_GROUP"]             # blocks per packed GLWE
PACK_KEY_WORDS = _K["FHS_PACK_KEY_WORDS"]
REKEY_KEY_WORDS = _K["FHS_REKEY_KEY_WORDS"]
SELECT_QUERY_BIT_WORDS = _K["FHS_SELECT_QUERY_BIT_WORDS"]       # u64 words of one index bit's GGSW
SELECT_REKEY_COST = _K["FHS_SELECT_REKEY_COST"]
SELECT_SEEDED_BIT_WORDS = _K["FHS_SELECT_SEEDED_BIT_WORDS"]     # body words of one index bit of a seeded query
SELECT_FORM_FULL, SELECT_FORM_SEEDED = _K["FHS_SELECT_FORM_FULL"], _K["FHS_SELECT_FORM_SEEDED"]
SELECT_MAX_BATCH = _K["FHS_SELECT_MAX_BATCH"]
SELECT_BATCH_MAX_BYTES = _K["FHS_SELECT_BATCH_MAX_BYTES"]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _coded(err, code):
    err.code = code
    return err


class Context:
    """fhs_ctx: one per GPU.  Replaces the tfhe::integer::ServerKey held by
    MyServerKey (src/server_key/mod.rs:13-16)."""

    def __init__(self, device_id=0, planner=False):
        self._L = lib()
        if not planner:
            check_single_hip_runtime()     # a second HIP runtime mapped since the library was loaded: refuse, do not crash
        h = C.c_void_p()
        if planner:        # fhs_ctx_create_planner: records and levelises DAGs (statistics only), computes nothing
            rc = self._L.fhs_ctx_create_planner(C.byref(h))
        else:
            rc = self._L.fhs_ctx_create(int(device_id), C.byref(h))
        self._h = h
        if rc != 0:
            msg = self._L.fhs_last_error(h).decode() if h else "allocation failed"
            if h:
                self._L.fhs_ctx_destroy(h)
            self._h = None
            raise FhsError("fhs_ctx_create failed (%d): %s" % (rc, msg))

    def close(self):
        if getattr(self, "_h", None):
            self._L.fhs_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            # raised without a local name for it: a frame that holds its own exception closes a cycle through the
            # traceback, and the handles the failed call was given would then live until the next garbage collection
            raise _coded(FhsError("fhs error %d: %s" % (rc, self._L.fhs_last_error(self._h).decode())), rc)

    ARITH_EXACT_NTT = _K["FHS_ARITH_EXACT_NTT"]
    ARITH_F64_FFT = _K["FHS_ARITH_F64_FFT"]
    ARITH_F64_FFT_MB2 = _K["FHS_ARITH_F64_FFT_MB2"]
    ARITH_EXACT_NTT_MB2 = _K["FHS_ARITH_EXACT_NTT_MB2"]

    def set_arithmetic(self, arith):
        """fhs_set_arithmetic: 0 ARITH_EXACT_NTT (default), 1 ARITH_F64_FFT, 2 ARITH_F64_FFT_MB2 (select before
        load_server_key; mode 2 also needs load_multibit_key)."""
        self._check(self._L.fhs_set_arithmetic(self._h, int(arith)))

    def set_launch_chunk(self, arith, n):
        """fhs_set_launch_chunk: ciphertexts per blind-rotation launch of that arithmetic (0 = whole batch)."""
        self._check(self._L.fhs_set_launch_chunk(self._h, int(arith), int(n)))

    def set_fft4_max_batch(self, n):
        """fhs_set_fft4_max_batch: batches <= n use the 4-wavefront FFT kernel (default 512)."""
        self._check(self._L.fhs_set_fft4_max_batch(self._h, int(n)))

    @property
    def arithmetic(self):
        return int(self._L.fhs_get_arithmetic(self._h))

    def load_server_key(self, bsk, ksk):
        bsk = np.ascontiguousarray(bsk, np.uint64)
        ksk = np.ascontiguousarray(ksk, np.uint64)
        assert bsk.size == 742 * 4 * 2048 and ksk.size == 2048 * 5 * 743
        self._check(self._L.fhs_load_server_key(self._h, _ptr(bsk), _ptr(ksk)))

    def load_compressed_server_key(self, seed, bsk_bodies, ksk_bodies):
        """fhs_load_compressed_server_key: the seeded masks are regenerated on the device."""
        seed = np.ascontiguousarray(seed, np.uint32)
        bsk_bodies = np.ascontiguousarray(bsk_bodies, np.uint64)
        ksk_bodies = np.ascontiguousarray(ksk_bodies, np.uint64)
        assert seed.size == 8 and bsk_bodies.size == 742 * 2 * 2048 and ksk_bodies.size == 2048 * 5
        self._check(self._L.fhs_load_compressed_server_key(self._h, _ptr(seed), _ptr(bsk_bodies), _ptr(ksk_bodies)))

    def chacha20_device(self, key, counter, nonce, n):
        """fhs_debug_chacha20_device: n 64-bit draws of the device ChaCha20 (the values of fhs_chacha20_stream)."""
        key = np.ascontiguousarray(key, np.uint32)
        nonce = np.ascontiguousarray(nonce, np.uint32)
        assert key.size == 8 and nonce.size == 3
        out = np.zeros(n, np.uint64)
        self._check(self._L.fhs_debug_chacha20_device(self._h, _ptr(key), int(counter), _ptr(nonce), _ptr(out), n))
        return out

    def blind_rotate_batch(self, ks, lut_idx, luts):
        """fhs_debug_blind_rotate_batch: blind rotation + sample extraction from given keyswitched LWEs [B, 743]."""
        ks = np.ascontiguousarray(ks, np.uint64).reshape(-1, 743)
        luts = np.ascontiguousarray(luts, np.uint64).reshape(-1, POLY_N)
        lut_idx = np.ascontiguousarray(lut_idx, np.uint32)
        out = np.zeros((ks.shape[0], BIG_CT), np.uint64)
        self._check(self._L.fhs_debug_blind_rotate_batch(self._h, _ptr(ks), _ptr(lut_idx), _ptr(luts), luts.shape[0],
                                                         _ptr(out), ks.shape[0]))
        return out

    def load_multibit_key(self, bsk_mb2):
        """fhs_load_multibit_key: pair key of ARITH_F64_FFT_MB2, after load_server_key in arithmetic 1 or 2."""
        bsk_mb2 = np.ascontiguousarray(bsk_mb2, np.uint64)
        assert bsk_mb2.size == 371 * 3 * 4 * 2048
        self._check(self._L.fhs_load_multibit_key(self._h, _ptr(bsk_mb2)))

    def load_packing_key(self, key):
        """fhs_load_packing_key: the 11 automorphism keyswitch keys of the packed download, after load_server_key."""
        key = np.ascontiguousarray(key, np.uint64)
        assert key.size == PACK_KEY_WORDS
        self._check(self._L.fhs_load_packing_key(self._h, _ptr(key)))

    def load_rekey_key(self, key):
        """fhs_load_rekey_key: the string store's keyswitch key to another client key, after load_server_key; None
        unloads it."""
        if key is not None:
            key = np.ascontiguousarray(key, np.uint64)
            assert key.size == REKEY_KEY_WORDS
        self._check(self._L.fhs_load_rekey_key(self._h, None if key is None else _ptr(key)))

    def rekey_device(self, mask32, body32, n_blocks):
        """fhs_debug_rekey_device: the re-key kernel on raw words of any block count -> (mask32, body32), the arguments
        and results of rekey_host."""
        g = (n_blocks + PACK_GROUP - 1) // PACK_GROUP
        mask32 = np.ascontiguousarray(mask32, np.uint32).reshape(g, POLY_N)
        body32 = np.ascontiguousarray(body32, np.uint32).reshape(n_blocks)
        m_out, b_out = np.zeros((g, POLY_N), np.uint32), np.zeros(n_blocks, np.uint32)
        self._check(self._L.fhs_debug_rekey_device(self._h, _ptr(mask32), _ptr(body32), n_blocks, _ptr(m_out), _ptr(b_out)))
        return m_out, b_out

    def select_device(self, query, mask32, body32, n_blocks, row_chars):
        """fhs_debug_select_device: the select's kernels on the raw words of a whole entry -> (mask32[2048],
        body32[4 row_chars]), the arguments and results of select_host."""
        query, bits, mask32, body32 = _select_args(query, mask32, body32, n_blocks)
        m_out, b_out = np.zeros(POLY_N, np.uint32), np.zeros(4 * row_chars, np.uint32)
        self._check(self._L.fhs_debug_select_device(self._h, _ptr(query), bits, _ptr(mask32), _ptr(body32), n_blocks, row_chars,
                                                    _ptr(m_out), _ptr(b_out)))
        return m_out, b_out

    def select_seeded_device(self, q, mask32, body32, n_blocks, row_chars):
        """fhs_debug_select_seeded_device: select_device with a SeededSelectQuery."""
        g = (n_blocks + PACK_GROUP - 1) // PACK_GROUP
        mask32 = np.ascontiguousarray(mask32, np.uint32).reshape(g, POLY_N)
        body32 = np.ascontiguousarray(body32, np.uint32).reshape(n_blocks)
        m_out, b_out = np.zeros(POLY_N, np.uint32), np.zeros(4 * row_chars, np.uint32)
        self._check(self._L.fhs_debug_select_seeded_device(self._h, _ptr(q.seed), _ptr(q.bodies), q.bits, _ptr(mask32),
                                                           _ptr(body32), n_blocks, row_chars, _ptr(m_out), _ptr(b_out)))
        return m_out, b_out

    def select_query_device(self, query):
        """fhs_debug_select_query_device: the conversion kernel alone on a full-form query (an array) or a
        SeededSelectQuery -> the transform-domain doubles [bits][8][2 primes][2048]."""
        if isinstance(query, SeededSelectQuery):
            form, seed, words, bits = SELECT_FORM_SEEDED, _ptr(query.seed), query.bodies, query.bits
        else:
            words = np.ascontiguousarray(query, np.uint64)
            assert words.size % SELECT_QUERY_BIT_WORDS == 0
            form, seed, bits = SELECT_FORM_FULL, None, words.size // SELECT_QUERY_BIT_WORDS
        out = np.zeros((bits, 8, 2, POLY_N), np.float64)
        self._check(self._L.fhs_debug_select_query_device(self._h, form, seed, _ptr(words), bits, _ptr(out)))
        return out

    def rekey_packed_device(self, mask64, body64, n_blocks):
        """fhs_debug_rekey_packed_device: the recipient download's kernel on raw 64-bit GLWEs of any block count ->
        (mask16, body16), the arguments and results of rekey_packed_host."""
        g = (n_blocks + PACK_GROUP - 1) // PACK_GROUP
        mask64 = np.ascontiguousarray(mask64, np.uint64).reshape(g, POLY_N)
        body64 = np.ascontiguousarray(body64, np.uint64).reshape(g, POLY_N)
        m_out, b_out = np.zeros((g, POLY_N), np.uint16), np.zeros(n_blocks, np.uint16)
        self._check(self._L.fhs_debug_rekey_packed_device(self._h, _ptr(mask64), _ptr(body64), n_blocks, _ptr(m_out), _ptr(b_out)))
        return m_out, b_out

    def pbs_batch(self, cts, lut_idx, luts):
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, BIG_CT)
        luts = np.ascontiguousarray(luts, np.uint64).reshape(-1, POLY_N)
        lut_idx = np.ascontiguousarray(lut_idx, np.uint32)
        B = cts.shape[0]
        assert lut_idx.size == B
        out = np.zeros((B, BIG_CT), np.uint64)
        self._check(self._L.fhs_pbs_batch(self._h, _ptr(cts), _ptr(lut_idx), _ptr(luts), luts.shape[0],
                                          _ptr(out), B))
        return out

    def pbs_batch_shifted(self, cts, lut_idx, luts, shifts):
        """fhs_pbs_batch_shifted: ONE blind rotation per input, one sample extraction per shift -> [B, S, 2049]; row
        (b, s) = what a bootstrap of (cts[b] + shifts[b][s] * Delta) yields (message units 0..31)."""
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, BIG_CT)
        luts = np.ascontiguousarray(luts, np.uint64).reshape(-1, POLY_N)
        lut_idx = np.ascontiguousarray(lut_idx, np.uint32)
        B = cts.shape[0]
        shifts = np.ascontiguousarray(shifts, np.uint32).reshape(B, -1)
        out = np.zeros((B, shifts.shape[1], BIG_CT), np.uint64)
        self._check(self._L.fhs_pbs_batch_shifted(self._h, _ptr(cts), _ptr(lut_idx), _ptr(luts), luts.shape[0],
                                                  _ptr(shifts), shifts.shape[1], _ptr(out), B))
        return out

    def set_rotation_sharing(self, on=True):
        self._check(self._L.fhs_set_rotation_sharing(self._h, int(bool(on))))

    def keyswitch_modswitch_batch(self, cts):
        cts = np.ascontiguousarray(cts, np.uint64).reshape(-1, BIG_CT)
        B = cts.shape[0]
        out = np.zeros((B, SMALL_CT), np.uint32)
        self._check(self._L.fhs_keyswitch_modswitch_batch(self._h, _ptr(cts), _ptr(out), B))
        return out

    def pbs_batch_device(self, d_in, d_lut_idx, d_luts, d_out, B, stream=0):
        """All arguments are raw device pointers (ints), e.g. torch tensor.data_ptr()."""
        self._check(self._L.fhs_pbs_batch_device(self._h, C.c_void_p(d_in), C.c_void_p(d_lut_idx),
                                                 C.c_void_p(d_luts), C.c_void_p(d_out), int(B),
                                                 C.c_void_p(stream)))

    def kernel_timing(self, reset=False):
        br, ks = C.c_double(), C.c_double()
        nb, nk, units = C.c_uint64(), C.c_uint64(), C.c_uint64()
        narrow = self.kernel_timing_kind(2)                     # read before a reset
        self._check(self._L.fhs_kernel_timing(self._h, int(reset), C.byref(br), C.byref(ks), C.byref(nb),
                                              C.byref(nk), C.byref(units)))
        return {"blind_rotate_ms": br.value, "keyswitch_ms": ks.value, "n_blind_rotate": nb.value,
                "n_keyswitch": nk.value, "pbs_in_launches": units.value,
                "fft4_ms": narrow[0], "n_fft4": narrow[1], "pbs_in_fft4": narrow[2]}

    def kernel_timing_kind(self, kind):
        """(average ms, launches, PBS) of one kernel class: 0 wide blind rotation, 1 keyswitch, 2 4-wavefront FFT,
        3 the launches of class 0 that ran the shifted-accumulator instantiation of the 2-wavefront FFT kernel."""
        ms, n, u = C.c_double(), C.c_uint64(), C.c_uint64()
        self._check(self._L.fhs_kernel_timing_kind(self._h, int(kind), C.byref(ms), C.byref(n), C.byref(u)))
        return ms.value, n.value, u.value


# ---------------------------------------------------------------------------------------------
# Mirror of the reference's types: MyClientKey (src/client_key.rs), FheAsciiChar / FheString
# (src/ciphertext), MyServerKey (src/server_key/mod.rs).  Same method names and argument meaning;
# `public_parameters` is accepted and ignored by every operation, like the reference's dead parameter;
# PublicParameters itself is real: it encrypts without the client key (PublicParameters.encrypt).
# ---------------------------------------------------------------------------------------------
CHAR_WORDS = _K["FHS_CHAR_WORDS"]
MAX_FIND_LENGTH = _K["FHS_MAX_FIND_LENGTH"]
MAX_REPETITIONS = _K["FHS_MAX_REPETITIONS"]
MAX_FIND_LENGTH_WIDE = _K["FHS_MAX_FIND_LENGTH_WIDE"]
WIDE_ABSENT = _K["FHS_WIDE_ABSENT"]
STRING_PADDING = 1
MODE_AS_WRITTEN = _K["FHS_MODE_AS_WRITTEN"]
MODE_FUSED = _K["FHS_MODE_FUSED"]


class MyClientKey:
    """Host-CPU client key (keygen / encrypt / decrypt), like the reference's.

    MyClientKey() draws everything from a ChaCha20 generator keyed with OS entropy (fhs_client_create), like the
    reference's OS-seeded tfhe-rs CSPRNG.  MyClientKey(seed) is the TEST / BENCHMARK constructor
    (fhs_client_create_insecure_seeded): reproducible keys, identical on every rank, never for real data."""

    def __init__(self, seed=None, _handle=None):
        import threading
        self._L = lib()
        self._scratch, self._scratch_lock = None, threading.Lock()
        if _handle is not None:
            self._h = _handle
            return
        h = C.c_void_p()
        if seed is None:
            rc = self._L.fhs_client_create(C.byref(h))
        else:
            rc = self._L.fhs_client_create_insecure_seeded(int(seed), C.byref(h))
        if rc != 0:
            raise FhsError("fhs_client_create failed (%d)" % rc)
        self._h = h

    def save(self, path, server_key_only=False):
        """Key file (include/fhestring_hip.h "key files"): raw little-endian u64 arrays + 64-byte header."""
        if self._L.fhs_client_save(self._h, str(path).encode(), int(server_key_only)) != 0:
            raise FhsError("cannot write key file %s" % path)

    def save_multibit_key(self, path):
        """fhs_client_save_multibit_key: kind 3 file with the pair key of the two-key-bits-per-product arithmetics."""
        if self._L.fhs_client_save_multibit_key(self._h, str(path).encode()) != 0:
            raise FhsError("cannot write pair key file %s" % path)

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        if lib().fhs_client_load(str(path).encode(), C.byref(h)) != 0:
            raise FhsError("cannot read client key file %s" % path)
        return cls(_handle=h)

    @classmethod
    def from_params(cls, params=None, num_blocks=4, seed=None):   # client_key.rs:30-35 (seed: tests only)
        assert num_blocks == 4
        return cls(seed)

    def close(self):
        if getattr(self, "_h", None):
            self._L.fhs_client_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bsk(self):
        return np.ctypeslib.as_array(self._L.fhs_client_bsk(self._h), shape=(742 * 4 * 2048,))

    def ksk(self):
        return np.ctypeslib.as_array(self._L.fhs_client_ksk(self._h), shape=(2048 * 5 * 743,))

    def bsk_mb2(self):
        """fhs_client_bsk_mb2: pair key of ARITH_F64_FFT_MB2 (generated on first use)."""
        return np.ctypeslib.as_array(self._L.fhs_client_bsk_mb2(self._h), shape=(371 * 3 * 4 * 2048,))

    def secret_keys(self):
        lwe = np.zeros(742, np.uint64)
        glwe = np.zeros(2048, np.uint64)
        self._L.fhs_client_secret_keys(self._h, _ptr(lwe), _ptr(glwe))
        return lwe, glwe

    def get_server_key(self, device_id=0, arith=0):                      # client_key.rs:37-39
        return MyServerKey.from_client_key(self, device_id, arith)

    def encrypt_char_raw(self, v):
        out = np.zeros((4, BIG_CT), np.uint64)
        self._L.fhs_client_encrypt_char(self._h, int(v) & 255, _ptr(out))
        return out

    def encrypt_str_raw(self, text, padding, out=None):
        data = text.encode("ascii") if isinstance(text, str) else bytes(text)
        if out is None:
            out = np.empty((len(data) + padding, 4, BIG_CT), np.uint64)  # every word is written by the call
        rc = self._L.fhs_client_encrypt_str(self._h, data, len(data), int(padding), _ptr(out))
        if rc != 0:
            raise AssertionError("The input string must only contain ascii letters and not include null characters")
        return out

    def decrypt_char_raw(self, blocks):
        v = C.c_uint8()
        blocks = np.ascontiguousarray(blocks, np.uint64)
        self._L.fhs_client_decrypt_char(self._h, _ptr(blocks), C.byref(v))
        return v.value

    def decrypt_str_raw(self, chars):
        chars = np.ascontiguousarray(chars, np.uint64).reshape(-1, 4, BIG_CT)
        buf = C.create_string_buffer(chars.shape[0] + 1)
        n = C.c_size_t()
        self._L.fhs_client_decrypt_str(self._h, _ptr(chars), chars.shape[0], buf, C.byref(n))
        return buf.raw[:n.value].decode("ascii")

    def encrypt_compressed(self, string, padding):
        """fhs_client_encrypt_str_compressed: the string's masks come from a fresh public seed, only the bodies are kept
        (32 B per character instead of 65 568 B)."""
        data = string.encode("ascii") if isinstance(string, str) else bytes(string)
        seed = np.zeros(8, np.uint32)
        bodies = np.empty((len(data) + padding, 4), np.uint64)
        rc = self._L.fhs_client_encrypt_str_compressed(self._h, data, len(data), int(padding), _ptr(seed), _ptr(bodies))
        if rc != 0:
            raise AssertionError("The input string must only contain ascii letters and not include null characters")
        return CompressedFheString(seed, bodies)

    def compressed_server_key(self):
        """fhs_client_compressed_server_key: (seed[8] u32, bsk_bodies[742][2][2048], ksk_bodies[2048][5]) of a second
        server key of this client whose masks come from the public seed (generated on first use)."""
        seed = np.zeros(8, np.uint32)
        bb = np.empty((742, 2, 2048), np.uint64)
        kb = np.empty((2048, 5), np.uint64)
        if self._L.fhs_client_compressed_server_key(self._h, _ptr(seed), _ptr(bb), _ptr(kb)) != 0:
            raise FhsError("fhs_client_compressed_server_key failed")
        return seed, bb, kb

    def save_compressed_server_key(self, path):
        """fhs_client_save_compressed_server_key: kind 4 key file (seed + bodies, 24 395 872 B)."""
        if self._L.fhs_client_save_compressed_server_key(self._h, str(path).encode()) != 0:
            raise FhsError("cannot write compressed key file %s" % path)

    def packing_key(self):
        """fhs_client_packing_key: the automorphism keyswitch keys of the packed result download (generated on first
        use, ~1 MB)."""
        return np.ctypeslib.as_array(self._L.fhs_client_packing_key(self._h), shape=(PACK_KEY_WORDS,))

    def save_packing_key(self, path):
        """fhs_client_save_packing_key: kind 5 key file; it travels beside a kind 1 / 2 / 4 file."""
        if self._L.fhs_client_save_packing_key(self._h, str(path).encode()) != 0:
            raise FhsError("cannot write packing key file %s" % path)

    def rekey_key(self, to):
        """fhs_client_rekey_key: the key that moves parked store entries of THIS client under the key of `to` (another
        MyClientKey); a fresh key per call, [2][mask, body][2048] words."""
        key = np.empty(REKEY_KEY_WORDS, np.uint64)
        if self._L.fhs_client_rekey_key(self._h, to._h, _ptr(key)) != 0:
            raise FhsError("fhs_client_rekey_key failed")
        return key

    def select_query(self, index, n_chars, row_chars, seeded=False):
        """fhs_client_select_query: the bits of row `index` of a table of n_chars characters in rows of row_chars, as GGSW
        ciphertexts under this client's key -> (query[bits][4][mask, body][2048] u64, bits); a fresh query per call.
        seeded=True: fhs_client_select_query_seeded -> SeededSelectQuery(seed, bodies[bits][4][2048], bits), half the size."""
        bits = select_bits(n_chars, row_chars)
        if bits == 0:
            raise ValueError("no table of %d characters in rows of %d can be selected from" % (n_chars, row_chars))
        if seeded:
            seed, bodies = np.zeros(8, np.uint32), np.empty((bits, 4, POLY_N), np.uint64)
            if self._L.fhs_client_select_query_seeded(self._h, int(index), bits, _ptr(seed), _ptr(bodies)) != 0:
                raise FhsError("fhs_client_select_query_seeded failed")
            return SeededSelectQuery(seed, bodies, bits)
        query = np.empty((bits, 4, 2, POLY_N), np.uint64)
        if self._L.fhs_client_select_query(self._h, int(index), bits, _ptr(query)) != 0:
            raise FhsError("fhs_client_select_query failed")
        return query, bits

    def save_rekey_key(self, to, path):
        """fhs_client_save_rekey_key: kind 7 key file with a fresh re-key key from this client to `to`."""
        if self._L.fhs_client_save_rekey_key(self._h, to._h, str(path).encode()) != 0:
            raise FhsError("cannot write re-key key file %s" % path)

    def encrypt_blocks_raw(self, values):
        """fhs_client_encrypt_blocks (diagnostic): one block per value mod 32, carry bits included: [n][2049]."""
        values = np.ascontiguousarray(values, np.uint8)
        out = np.empty((values.size, BIG_CT), np.uint64)
        if self._L.fhs_client_encrypt_blocks(self._h, _ptr(values), values.size, _ptr(out)) != 0:
            raise FhsError("fhs_client_encrypt_blocks failed")
        return out

    def decrypt_packed_blocks(self, p):
        """Every block of a PackedFheString mod 32 (message, carry and padding bits): [4 n] u8."""
        out = np.zeros(4 * len(p), np.uint8)
        if self._L.fhs_client_decrypt_packed_blocks_at(self._h, _ptr(p.mask16), _ptr(p.body16), p.first_coef, 4 * len(p),
                                                       _ptr(out)) != 0:
            raise FhsError("fhs_client_decrypt_packed_blocks_at failed")
        return out

    def decrypt_packed(self, p):
        """fhs_client_decrypt_packed_str_at: MyClientKey.decrypt on a PackedFheString, whole or a window of a parked
        entry (truncates at the first NUL)."""
        buf = C.create_string_buffer(len(p) + 1)
        n = C.c_size_t()
        if self._L.fhs_client_decrypt_packed_str_at(self._h, _ptr(p.mask16), _ptr(p.body16), p.first_coef, len(p), buf,
                                                    C.byref(n)) != 0:
            raise FhsError("fhs_client_decrypt_packed_str_at failed")
        return buf.raw[:n.value].decode("ascii")

    def public_key(self):
        """fhs_client_public_key: (seed[8] u32, body[2048] u64) of the client's public key (generated on first use)."""
        seed = np.zeros(8, np.uint32)
        body = np.empty(2048, np.uint64)
        if self._L.fhs_client_public_key(self._h, _ptr(seed), _ptr(body)) != 0:
            raise FhsError("fhs_client_public_key failed")
        return seed, body

    def save_public_key(self, path):
        """fhs_client_save_public_key: kind 6 key file (seed + B, 16 480 B; no secret in it)."""
        if self._L.fhs_client_save_public_key(self._h, str(path).encode()) != 0:
            raise FhsError("cannot write public key file %s" % path)

    def get_public_parameters(self):                                                # client_key.rs:41-43
        return PublicParameters(*self.public_key())

    # reference-shaped API (server key needed to place ciphertexts on the device)
    def encrypt(self, string, padding, public_parameters=None, server_key=None):   # :45-65
        # the ciphertext only lives until fhs_upload_string has staged it: one scratch buffer per client, grown on demand
        # (a fresh 268 MB array per 4097-character string is 65 000 page faults before the first byte is encrypted)
        # ctypes releases the GIL inside fhs_client_encrypt_str / fhs_upload_string (the C side is thread-safe, per-call
        # streams): the scratch buffer is therefore guarded by a per-client lock -- two threads encrypting with one client
        # key take turns -- and a buffer that grew beyond 320 MB (more than BASELINE's largest string, 4097
        # characters = 268 MB) is dropped after use instead of staying pinned for the client's lifetime
        n = len(string) + padding
        with self._scratch_lock:
            if self._scratch is None or self._scratch.shape[0] < n:
                self._scratch = np.empty((max(n, 64), 4, BIG_CT), np.uint64)
            try:
                return server_key.upload_string(self.encrypt_str_raw(string, padding, out=self._scratch[:n]))
            finally:
                if self._scratch.nbytes > (320 << 20):
                    self._scratch = None

    def encrypt_no_padding(self, string, server_key=None):                         # :67-79
        return server_key.upload_string(self.encrypt_str_raw(string, 0)).chars

    def encrypt_char(self, v, server_key=None):                                    # :85-87
        return server_key.upload_char(self.encrypt_char_raw(v))

    def decrypt_char(self, ch):                                                    # :81-83
        return self.decrypt_char_raw(ch.download())

    def decrypt(self, fhe_string):                                                 # :89-106
        return self.decrypt_str_raw(fhe_string.download())

    def decrypt_u16(self, wide):
        """The integer of an FheU16 (find_wide, rfind_wide, len_wide, count_flags_wide)."""
        return self.decrypt_char(wide.lo) + 256 * self.decrypt_char(wide.hi)


class FheAsciiChar:
    """Handle of one lazily evaluated encrypted char (fheasciichar.rs:8-10)."""
    __slots__ = ("sk", "h")

    def __init__(self, sk, h):
        if not h:
            raise FhsError("null char handle: " + sk.ctx._L.fhs_last_error(sk.ctx._h).decode())
        self.sk = sk
        self.h = h

    def __del__(self):
        try:
            if self.h and self.sk.ctx._h:
                self.sk.ctx._L.fhs_release(self.sk.ctx._h, self.h)
        except Exception:
            pass

    @staticmethod
    def encrypt_trivial(value, public_parameters, server_key):           # :17-25
        return server_key.trivial(value)

    def _bin(self, name, other):
        L, c = self.sk.ctx._L, self.sk.ctx._h
        return FheAsciiChar(self.sk, getattr(L, "fhs_" + name)(c, self.h, other.h))

    def eq(self, o): return self._bin("eq", o)
    def ne(self, o): return self._bin("ne", o)
    def le(self, o): return self._bin("le", o)
    def lt(self, o): return self._bin("lt", o)
    def ge(self, o): return self._bin("ge", o)
    def gt(self, o): return self._bin("gt", o)
    def bitand(self, o): return self._bin("bitand", o)
    def bitor(self, o): return self._bin("bitor", o)
    def sub(self, o): return self._bin("sub", o)
    def add(self, o): return self._bin("add", o)

    def if_then_else(self, t, f):
        return FheAsciiChar(self.sk, self.sk.ctx._L.fhs_if_then_else(self.sk.ctx._h, self.h, t.h, f.h))

    def _un(self, name):
        return FheAsciiChar(self.sk, getattr(self.sk.ctx._L, "fhs_" + name)(self.sk.ctx._h, self.h))

    def flip(self): return self._un("flip")
    def is_whitespace(self): return self._un("is_whitespace")
    def is_uppercase(self): return self._un("is_uppercase")
    def is_lowercase(self): return self._un("is_lowercase")
    def clone(self): return self._un("clone")

    def sum_c2(self):
        """Noise of the handle in bootstrap-output variances (fhs_char_sum_c2): results come back at <= 4 except find's
        index (<= 57).  The figure stays with the handle across a download; a ciphertext that leaves the library takes
        it along (`download()` + `sum_c2()`), and `set_noise()` declares it after the upload on the other side."""
        v = C.c_uint64(0)
        self.sk.ctx._check(self.sk.ctx._L.fhs_char_sum_c2(self.sk.ctx._h, self.h, C.byref(v)))
        return int(v.value)

    def set_noise(self, sum_c2):
        """fhs_char_set_noise: this uploaded ciphertext is a result that was handed out at `sum_c2` (uploads count as 1)."""
        self.sk.ctx._check(self.sk.ctx._L.fhs_char_set_noise(self.sk.ctx._h, self.h, int(sum_c2)))
        return self

    def trivial_value(self):
        """The byte if every block of the handle is a trivial ciphertext (what constant folding left), else None."""
        t, v = C.c_int(0), C.c_uint8(0)
        self.sk.ctx._check(self.sk.ctx._L.fhs_trivial_value(self.sk.ctx._h, self.h, C.byref(t), C.byref(v)))
        return int(v.value) if t.value else None

    def download(self):
        out = np.zeros((4, BIG_CT), np.uint64)
        self.sk.flush()                      # (collective in level-parallel mode)
        self.sk.ctx._check(self.sk.ctx._L.fhs_download(self.sk.ctx._h, self.h, _ptr(out)))
        return out


class FheU16:
    """A 16-bit unsigned result as two ordinary chars: value = lo + 256 * hi (the _wide entry points of the C ABI)."""
    __slots__ = ("lo", "hi")

    def __init__(self, lo, hi):
        self.lo = lo
        self.hi = hi

    def trivial_value(self):
        """The integer if both halves folded to constants, else None."""
        lo, hi = self.lo.trivial_value(), self.hi.trivial_value()
        return None if lo is None or hi is None else lo + 256 * hi


class FheString:
    """Vec<FheAsciiChar> (fhestring.rs:6-9)."""

    def __init__(self, chars):
        self.chars = list(chars)

    def __len__(self):
        return len(self.chars)

    def __getitem__(self, i):
        return self.chars[i]

    def download(self):
        """[n][4][2049] words: the whole string with one gather + one copy per 2048 blocks (fhs_download_string)."""
        if not self.chars:
            return np.zeros((0, 4, BIG_CT), np.uint64)
        sk = self.chars[0].sk
        out = np.empty((len(self.chars), 4, BIG_CT), np.uint64)
        sk.ctx._check(sk.ctx._L.fhs_download_string(sk.ctx._h, _harr(self.chars), len(self.chars), _ptr(out)))
        return out


class CompressedFheString:
    """A seeded FheString: the public seed (8 x u32) and the body of every block ([n][4] u64); the masks follow from the
    seed (include/fhestring_hip.h, "compressed ciphertexts").  Serialised form: magic FHSCSTR1, n (u64), seed, bodies."""

    MAGIC = b"FHSCSTR1"

    def __init__(self, seed, bodies):
        self.seed = np.ascontiguousarray(seed, np.uint32).reshape(8)
        self.bodies = np.ascontiguousarray(bodies, np.uint64).reshape(-1, 4)

    def __len__(self):
        return self.bodies.shape[0]

    @property
    def nbytes(self):
        return 48 + self.bodies.nbytes

    def to_bytes(self):
        return self.MAGIC + np.uint64(len(self)).tobytes() + self.seed.tobytes() + self.bodies.tobytes()

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        if data[:8] != cls.MAGIC or len(data) < 48:
            raise ValueError("not a compressed FheString")
        n = int(np.frombuffer(data, np.uint64, 1, 8)[0])
        if len(data) != 48 + 32 * n:
            raise ValueError("compressed FheString of %d characters needs %d bytes, got %d" % (n, 48 + 32 * n, len(data)))
        return cls(np.frombuffer(data, np.uint32, 8, 16), np.frombuffer(data, np.uint64, 4 * n, 48))

    def _window(self, first_char, count):
        if count is None:
            count = len(self) - first_char
        assert 0 <= first_char and 0 <= count and first_char + count <= len(self)
        return first_char, count

    def expand(self, first_char=0, count=None):
        """fhs_expand_compressed_str: characters [first_char, first_char + count) as classic [count][4][2049] words."""
        first_char, count = self._window(first_char, count)
        out = np.empty((count, 4, BIG_CT), np.uint64)
        bodies = np.ascontiguousarray(self.bodies[first_char:first_char + count])
        if lib().fhs_expand_compressed_str(_ptr(self.seed), _ptr(bodies), count, first_char, _ptr(out)) != 0:
            raise FhsError("fhs_expand_compressed_str failed")
        return out

    def decompress(self, server_key, first_char=0, count=None):
        """Expands characters [first_char, first_char + count) on the server key's GPU -> FheString."""
        return server_key.upload_compressed_string(self, first_char, count)


class PublicParameters:
    """The reference's PublicParameters (src/ciphertext/public_parameters.rs): the client's public key and the number of
    blocks per character.  It holds no secret: anyone can encrypt() with it, and only the client key decrypts
    (include/fhestring_hip.h, "public-key encryption").  Serialised form: magic FHSPUBK1, seed, body (16 424 B)."""

    MAGIC = b"FHSPUBK1"
    num_blocks = 4

    def __init__(self, seed, body, _handle=None):
        self._L = lib()
        if _handle is None:
            seed = np.ascontiguousarray(seed, np.uint32).reshape(8)
            body = np.ascontiguousarray(body, np.uint64).reshape(2048)
            _handle = C.c_void_p()
            if self._L.fhs_public_key_create(_ptr(seed), _ptr(body), C.byref(_handle)) != 0:
                raise FhsError("fhs_public_key_create failed")
        self._h = _handle

    def close(self):
        if getattr(self, "_h", None):
            self._L.fhs_public_key_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def public_key(self):
        """(seed[8] u32, body[2048] u64)"""
        seed = np.zeros(8, np.uint32)
        body = np.empty(2048, np.uint64)
        if self._L.fhs_public_key_get(self._h, _ptr(seed), _ptr(body)) != 0:
            raise FhsError("fhs_public_key_get failed")
        return seed, body

    def to_bytes(self):
        seed, body = self.public_key
        return self.MAGIC + seed.tobytes() + body.tobytes()

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        if data[:8] != cls.MAGIC or len(data) != 8 + 32 + 2048 * 8:
            raise ValueError("not a serialised PublicParameters")
        return cls(np.frombuffer(data, np.uint32, 8, 8), np.frombuffer(data, np.uint64, 2048, 40))

    def save(self, path):
        """The kind 6 key file of fhs_client_save_public_key."""
        seed, body = self.public_key
        hdr = np.array([6, 742, 2048, 5, 3, 23, 6], np.uint64)
        with open(str(path), "wb") as f:
            f.write(b"FHSKEY01" + hdr.tobytes() + seed.tobytes() + body.tobytes())

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        if lib().fhs_public_key_load(str(path).encode(), C.byref(h)) != 0:
            raise FhsError("cannot read public key file %s (missing, truncated or not kind 6)" % path)
        return cls(None, None, _handle=h)

    def set_insecure_seed(self, seed):
        """TESTS ONLY (fhs_public_key_set_insecure_seed): reproducible encryption randomness."""
        if self._L.fhs_public_key_set_insecure_seed(self._h, int(seed)) != 0:
            raise FhsError("fhs_public_key_set_insecure_seed failed")

    def encrypt(self, string, padding):
        """fhs_public_encrypt_str: host only, no secret -> CompactFheString."""
        data = string.encode("ascii") if isinstance(string, str) else bytes(string)
        n = len(data) + int(padding)
        mw, bw = C.c_size_t(), C.c_size_t()
        self._L.fhs_public_str_words(n, C.byref(mw), C.byref(bw))
        mask32 = np.empty(max(1, mw.value), np.uint32)[:mw.value]
        body32 = np.empty(max(1, bw.value), np.uint32)[:bw.value]
        rc = self._L.fhs_public_encrypt_str(self._h, data, len(data), int(padding), _ptr(mask32), _ptr(body32))
        if rc != 0:
            raise AssertionError("The input string must only contain ascii letters and not include null characters")
        return CompactFheString(n, mask32, body32)


class CompactFheString:
    """A public-key encrypted FheString: one GLWE ciphertext per 2048 blocks (512 characters), every word at 32 bits --
    mask32[ceil(4n / 2048)][2048] and body32[4n] (include/fhestring_hip.h, "public-key encryption").  Serialised form:
    magic FHSPSTR1, n (u64), masks, bodies."""

    MAGIC = b"FHSPSTR1"

    def __init__(self, n, mask32, body32):
        self.n = int(n)
        self.mask32 = np.ascontiguousarray(mask32, np.uint32).reshape(-1, 2048)
        self.body32 = np.ascontiguousarray(body32, np.uint32).reshape(-1)
        assert self.mask32.shape[0] == (4 * self.n + 2047) // 2048 and self.body32.size == 4 * self.n

    def __len__(self):
        return self.n

    @property
    def nbytes(self):
        return 16 + self.mask32.nbytes + self.body32.nbytes

    def to_bytes(self):
        return self.MAGIC + np.uint64(self.n).tobytes() + self.mask32.tobytes() + self.body32.tobytes()

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        if data[:8] != cls.MAGIC or len(data) < 16:
            raise ValueError("not a compact FheString")
        n = int(np.frombuffer(data, np.uint64, 1, 8)[0])
        groups = (4 * n + 2047) // 2048
        if len(data) != 16 + 8192 * groups + 16 * n:
            raise ValueError("compact FheString of %d characters needs %d bytes, got %d"
                             % (n, 16 + 8192 * groups + 16 * n, len(data)))
        return cls(n, np.frombuffer(data, np.uint32, 2048 * groups, 16), np.frombuffer(data, np.uint32, 4 * n, 16 + 8192 * groups))

    def _window(self, first_char, count):
        if count is None:
            count = len(self) - first_char
        if not (0 <= first_char and 0 <= count and first_char + count <= len(self)):
            raise ValueError("window [%d, %d + %d) outside a string of %d characters" % (first_char, first_char, count, len(self)))
        return first_char, count

    def expand(self, first_char=0, count=None):
        """fhs_expand_public_str: characters [first_char, first_char + count) as classic [count][4][2049] words."""
        first_char, count = self._window(first_char, count)
        out = np.empty((count, 4, BIG_CT), np.uint64)
        if lib().fhs_expand_public_str(_ptr(self.mask32), _ptr(self.body32), self.n, first_char, count, _ptr(out)) != 0:
            raise FhsError("fhs_expand_public_str failed")
        return out


class PackedFheString:
    """A result string as it leaves the server packed: one 2048 x u16 GLWE mask per group of 512 characters and one u16
    body per block (include/fhestring_hip.h, "packed result download").  Serialised form: magic FHSPSTR1, n (u64), masks,
    bodies: 16 + 4096 * ceil(4 n / 2048) + 8 n bytes.
    A window of a parked entry (StoredString.download_packed) starts at coefficient first_coef of its first mask instead
    of 0: block i is coefficient (first_coef + i) % 2048 of mask (first_coef + i) // 2048, and the masks are those of
    the ceil((first_coef + 4 n) / 2048) covering groups.  With first_coef = 0 nothing changes, the bytes included; any
    other serialises as magic FHSPSTW1, n (u64), first_coef (u64), masks, bodies."""

    MAGIC = b"FHSPSTR1"
    MAGIC_WINDOW = b"FHSPSTW1"

    def __init__(self, n_chars, mask16, body16, first_coef=0):
        self.n_chars, self.first_coef = int(n_chars), int(first_coef)
        if self.first_coef % 4 or not 0 <= self.first_coef < PACK_GROUP:
            raise ValueError("first_coef is a multiple of 4 below %d, not %d" % (PACK_GROUP, self.first_coef))
        mask16, body16 = np.ascontiguousarray(mask16, np.uint16), np.ascontiguousarray(body16, np.uint16)
        g = self.groups(self.n_chars, self.first_coef)
        if mask16.size != g * POLY_N or body16.size != 4 * self.n_chars:
            raise ValueError("packed FheString of %d characters needs %d groups and %d bodies" % (self.n_chars, g, 4 * self.n_chars))
        self.mask16 = mask16.reshape(g, POLY_N)
        self.body16 = body16.reshape(4 * self.n_chars)

    @staticmethod
    def groups(n_chars, first_coef=0):
        return (first_coef + 4 * n_chars + PACK_GROUP - 1) // PACK_GROUP if n_chars else 0

    @classmethod
    def empty(cls, n_chars, first_coef=0):
        return cls(n_chars, np.zeros((cls.groups(n_chars, first_coef), POLY_N), np.uint16), np.zeros(4 * n_chars, np.uint16),
                   first_coef)

    def __len__(self):
        return self.n_chars

    @property
    def nbytes(self):
        return (24 if self.first_coef else 16) + self.mask16.nbytes + self.body16.nbytes

    def to_bytes(self):
        head = self.MAGIC + np.uint64(self.n_chars).tobytes()
        if self.first_coef:
            head = self.MAGIC_WINDOW + np.uint64(self.n_chars).tobytes() + np.uint64(self.first_coef).tobytes()
        return head + self.mask16.tobytes() + self.body16.tobytes()

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        window = data[:8] == cls.MAGIC_WINDOW
        head = 24 if window else 16
        if (data[:8] != cls.MAGIC and not window) or len(data) < head:
            raise ValueError("not a packed FheString")
        n = int(np.frombuffer(data, np.uint64, 1, 8)[0])
        first_coef = int(np.frombuffer(data, np.uint64, 1, 16)[0]) if window else 0
        if window and (first_coef % 4 or not 0 < first_coef < PACK_GROUP):
            raise ValueError("packed window: first_coef %d is not a non-zero multiple of 4 below %d" % (first_coef, PACK_GROUP))
        if n > (1 << 24):
            raise ValueError("packed FheString of %d characters" % n)
        g = cls.groups(n, first_coef)
        need = head + 2 * POLY_N * g + 8 * n
        if len(data) != need:
            raise ValueError("packed FheString of %d characters needs %d bytes, got %d" % (n, need, len(data)))
        return cls(n, np.frombuffer(data, np.uint16, POLY_N * g, head), np.frombuffer(data, np.uint16, 4 * n, head + 2 * POLY_N * g),
                   first_coef)


def pack_host(key, blocks):
    """fhs_pack_host: host reference of the packing; blocks [n][2049] -> 64-bit GLWEs (mask64, body64) [groups][2048]."""
    key = np.ascontiguousarray(key, np.uint64)
    blocks = np.ascontiguousarray(blocks, np.uint64).reshape(-1, BIG_CT)
    assert key.size == PACK_KEY_WORDS
    n = blocks.shape[0]
    g = (n + PACK_GROUP - 1) // PACK_GROUP
    mask64, body64 = np.zeros((g, POLY_N), np.uint64), np.zeros((g, POLY_N), np.uint64)
    if lib().fhs_pack_host(_ptr(key), _ptr(blocks), n, _ptr(mask64), _ptr(body64)) != 0:
        raise FhsError("fhs_pack_host failed")
    return mask64, body64


def pack_switch16(mask64, body64, n_blocks):
    """fhs_pack_switch16: the storage switch of the host reference -> PackedFheString (n_blocks a multiple of 4) or, for
    any other block count, the raw (mask16, body16)."""
    mask64 = np.ascontiguousarray(mask64, np.uint64)
    body64 = np.ascontiguousarray(body64, np.uint64)
    g = (n_blocks + PACK_GROUP - 1) // PACK_GROUP
    assert mask64.size == g * POLY_N and body64.size == g * POLY_N
    mask16, body16 = np.zeros((g, POLY_N), np.uint16), np.zeros(n_blocks, np.uint16)
    if lib().fhs_pack_switch16(_ptr(mask64), _ptr(body64), n_blocks, _ptr(mask16), _ptr(body16)) != 0:
        raise FhsError("fhs_pack_switch16 failed")
    return PackedFheString(n_blocks // 4, mask16, body16) if n_blocks % 4 == 0 else (mask16, body16)


def pack_switch32(mask64, body64, n_blocks):
    """fhs_pack_switch32: the string store's storage switch on the host, (x + 2^31) >> 32 -> CompactFheString (n_blocks a
    multiple of 4) or, for any other block count, the raw (mask32, body32)."""
    mask64 = np.ascontiguousarray(mask64, np.uint64)
    body64 = np.ascontiguousarray(body64, np.uint64)
    g = (n_blocks + PACK_GROUP - 1) // PACK_GROUP
    assert mask64.size == g * POLY_N and body64.size == g * POLY_N
    mask32, body32 = np.zeros((g, POLY_N), np.uint32), np.zeros(n_blocks, np.uint32)
    if lib().fhs_pack_switch32(_ptr(mask64), _ptr(body64), n_blocks, _ptr(mask32), _ptr(body32)) != 0:
        raise FhsError("fhs_pack_switch32 failed")
    return CompactFheString(n_blocks // 4, mask32, body32) if n_blocks % 4 == 0 else (mask32, body32)


def rekey_host(key, mask32, body32=None, n_blocks=None):
    """fhs_rekey_host: host reference of the store's re-key.  rekey_host(key, compact) -> CompactFheString under the new
    client key; rekey_host(key, mask32, body32, n_blocks) -> the raw (mask32, body32) of any block count."""
    key = np.ascontiguousarray(key, np.uint64)
    assert key.size == REKEY_KEY_WORDS
    compact = mask32 if isinstance(mask32, CompactFheString) else None
    if compact is not None:
        mask32, body32, n_blocks = compact.mask32, compact.body32, 4 * len(compact)
    g = (n_blocks + PACK_GROUP - 1) // PACK_GROUP
    mask32 = np.ascontiguousarray(mask32, np.uint32).reshape(g, POLY_N)
    body32 = np.ascontiguousarray(body32, np.uint32).reshape(n_blocks)
    m_out, b_out = np.zeros((g, POLY_N), np.uint32), np.zeros(n_blocks, np.uint32)
    if lib().fhs_rekey_host(_ptr(key), _ptr(mask32), _ptr(body32), n_blocks, _ptr(m_out), _ptr(b_out)) != 0:
        raise FhsError("fhs_rekey_host failed")
    return CompactFheString(n_blocks // 4, m_out, b_out) if compact is not None else (m_out, b_out)


def select_bits(n_chars, row_chars):
    """fhs_store_select_bits: index bits of a table of n_chars characters in rows of row_chars, 0 for a refused shape."""
    return int(lib().fhs_store_select_bits(int(n_chars), int(row_chars)))


class SeededSelectQuery:
    """A select query in its seeded form: the public seed (8 u32 words) of the masks and bodies[bits][4][2048]."""

    def __init__(self, seed, bodies, bits):
        self.seed = np.ascontiguousarray(seed, np.uint32).reshape(8)
        self.bodies = np.ascontiguousarray(bodies, np.uint64).reshape(int(bits), 4, POLY_N)
        self.bits = int(bits)


def expand_select_query(q):
    """fhs_expand_select_query: the full form [bits][4][mask, body][2048] of a SeededSelectQuery (public data only)."""
    out = np.empty((q.bits, 4, 2, POLY_N), np.uint64)
    if lib().fhs_expand_select_query(_ptr(q.seed), _ptr(q.bodies), q.bits, _ptr(out)) != 0:
        raise FhsError("fhs_expand_select_query failed")
    return out


def select_query_ntt_host(query):
    """fhs_select_query_ntt_host: the host's conversion of a full-form query to the transform domain, the doubles
    [bits][8][2 primes][2048] that Context.select_query_device must reproduce bit for bit."""
    query = np.ascontiguousarray(query, np.uint64)
    assert query.size % SELECT_QUERY_BIT_WORDS == 0
    bits = query.size // SELECT_QUERY_BIT_WORDS
    out = np.zeros((bits, 8, 2, POLY_N), np.float64)
    if lib().fhs_select_query_ntt_host(_ptr(query), bits, _ptr(out)) != 0:
        raise FhsError("fhs_select_query_ntt_host failed")
    return out


def select_batch_bytes(n_chars, row_chars, n):
    """fhs_store_select_batch_bytes: workspace of a batch of n queries, 0 for a refused shape or n."""
    return int(lib().fhs_store_select_batch_bytes(int(n_chars), int(row_chars), int(n)))


def _select_args(query, mask32, body32, n_blocks):
    query = np.ascontiguousarray(query, np.uint64)
    assert query.size % SELECT_QUERY_BIT_WORDS == 0
    g = (n_blocks + PACK_GROUP - 1) // PACK_GROUP
    return (query, query.size // SELECT_QUERY_BIT_WORDS, np.ascontiguousarray(mask32, np.uint32).reshape(g, POLY_N),
            np.ascontiguousarray(body32, np.uint32).reshape(n_blocks))


def select_host(query, mask32, body32=None, n_blocks=None, row_chars=None):
    """fhs_store_select_host: host reference of StoredString.select.  select_host(query, compact, row_chars=r) ->
    CompactFheString of the selected row; select_host(query, mask32, body32, n_blocks, row_chars) -> the raw
    (mask32[2048], body32[4 row_chars])."""
    compact = mask32 if isinstance(mask32, CompactFheString) else None
    if compact is not None:
        mask32, body32, n_blocks = compact.mask32, compact.body32, 4 * len(compact)
    query, bits, mask32, body32 = _select_args(query, mask32, body32, n_blocks)
    m_out, b_out = np.zeros((1, POLY_N), np.uint32), np.zeros(4 * row_chars, np.uint32)
    rc = lib().fhs_store_select_host(_ptr(query), bits, _ptr(mask32), _ptr(body32), n_blocks, row_chars, _ptr(m_out), _ptr(b_out))
    if rc != 0:
        raise FhsError("fhs_store_select_host failed (%d)" % rc)
    return CompactFheString(row_chars, m_out, b_out) if compact is not None else (m_out[0], b_out)


def rekey_packed_host(key, mask64, body64, n_blocks):
    """fhs_rekey_packed_host: host reference of the packed download for a recipient.  The 64-bit GLWEs of pack_host (or of
    download_packed(wide=True)) -> PackedFheString under the recipient's key (n_blocks a multiple of 4) or, for any other
    block count, the raw (mask16, body16)."""
    key = np.ascontiguousarray(key, np.uint64)
    assert key.size == REKEY_KEY_WORDS
    g = (n_blocks + PACK_GROUP - 1) // PACK_GROUP
    mask64 = np.ascontiguousarray(mask64, np.uint64).reshape(g, POLY_N)
    body64 = np.ascontiguousarray(body64, np.uint64).reshape(g, POLY_N)
    mask16, body16 = np.zeros((g, POLY_N), np.uint16), np.zeros(n_blocks, np.uint16)
    if lib().fhs_rekey_packed_host(_ptr(key), _ptr(mask64), _ptr(body64), n_blocks, _ptr(mask16), _ptr(body16)) != 0:
        raise FhsError("fhs_rekey_packed_host failed")
    return PackedFheString(n_blocks // 4, mask16, body16) if n_blocks % 4 == 0 else (mask16, body16)


def store_packed_words(first_char, count):
    """fhs_store_packed_words -> (mask_words, body_words, first_coef) of the windowed packed form."""
    m, b, f = C.c_size_t(), C.c_size_t(), C.c_uint32()
    lib().fhs_store_packed_words(int(first_char), int(count), C.byref(m), C.byref(b), C.byref(f))
    return int(m.value), int(b.value), int(f.value)


def store_packed_host(key, compact, first_char=0, count=None):
    """fhs_store_packed_host: host reference of StoredString.download_packed.  `compact`: the whole entry as export()
    gives it (a CompactFheString); key: the re-key key of a recipient download, None for the entry's own key ->
    PackedFheString of characters [first_char, first_char + count)."""
    first_char, count = compact._window(first_char, count)
    if key is not None:
        key = np.ascontiguousarray(key, np.uint64)
        assert key.size == REKEY_KEY_WORDS
    p = PackedFheString.empty(count, store_packed_words(first_char, count)[2])
    if lib().fhs_store_packed_host(None if key is None else _ptr(key), _ptr(compact.mask32), _ptr(compact.body32), 4 * len(compact),
                                   first_char, count, _ptr(p.mask16), _ptr(p.body16)) != 0:
        raise FhsError("fhs_store_packed_host failed")
    return p


STORE_MAX_CYCLES = _K["FHS_STORE_MAX_CYCLES"]
STORE_MAX_REKEYS = _K["FHS_STORE_MAX_REKEYS"]
TRIM_RELEASE, TRIM_COMPACT = _K["FHS_TRIM_RELEASE"], _K["FHS_TRIM_COMPACT"]
STORE_META_MAGIC = b"FHSSMET1"


def store_meta_word(var=1, cycles=0, group=0):
    """One meta word of fhs_store_export / fhs_store_import: bits 0-15 the noise figure, 16-23 the packing cycles,
    32-63 the entry-local rotation group (0 = none)."""
    return np.uint64(int(var) | int(cycles) << 16 | int(group) << 32)


def store_export_to_bytes(compact, meta):
    """Serialised form of an exported entry: the CompactFheString bytes, then magic FHSSMET1, n (u64) and 4n meta words."""
    meta = np.ascontiguousarray(meta, np.uint64).reshape(-1)
    assert meta.size == 4 * len(compact)
    return compact.to_bytes() + STORE_META_MAGIC + np.uint64(len(compact)).tobytes() + meta.tobytes()


def store_export_from_bytes(data):
    """-> (CompactFheString, meta[4n]) of store_export_to_bytes."""
    data = bytes(data)
    if data[:8] != CompactFheString.MAGIC or len(data) < 16:
        raise ValueError("not an exported store entry")
    n = int(np.frombuffer(data, np.uint64, 1, 8)[0])
    cut = 16 + 8192 * ((4 * n + 2047) // 2048) + 16 * n
    if n > (1 << 24) or len(data) != cut + 16 + 32 * n or data[cut:cut + 8] != STORE_META_MAGIC or \
            int(np.frombuffer(data, np.uint64, 1, cut + 8)[0]) != n:
        raise ValueError("exported store entry of %d characters: wrong size or meta header" % n)
    return CompactFheString.from_bytes(data[:cut]), np.frombuffer(data, np.uint64, 4 * n, cut + 16).copy()


class StoredString:
    """One entry of a context's device-resident string store (include/fhestring_hip.h): the string parked in HBM in the
    compact format, 34 B per character, read back whole or by window with get()."""

    def __init__(self, sk, entry_id):
        self.sk, self.id = sk, int(entry_id)

    def _info(self):
        n, b = C.c_size_t(), C.c_size_t()
        self.sk.ctx._check(self.sk.ctx._L.fhs_store_info(self.sk.ctx._h, self.id, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def __len__(self):
        return self._info()[0]

    @property
    def device_bytes(self):
        return self._info()[1]

    def get(self, first_char=0, count=None):
        """fhs_store_get: characters [first_char, first_char + count) as a fresh FheString (needs no key)."""
        if count is None:
            count = len(self) - first_char
        hs = (C.c_uint64 * max(1, count))()
        self.sk.ctx._check(self.sk.ctx._L.fhs_store_get(self.sk.ctx._h, self.id, int(first_char), int(count), hs))
        return FheString([FheAsciiChar(self.sk, hs[i]) for i in range(count)])

    def drop(self):
        self.sk.ctx._check(self.sk.ctx._L.fhs_store_drop(self.sk.ctx._h, self.id))

    def rekey(self, copy=False):
        """fhs_store_rekey with the context's re-key key (MyServerKey.load_rekey_key): in place -> self, or copy=True ->
        a new StoredString under the other client's key while this one stays as it is."""
        if not copy:
            self.sk.ctx._check(self.sk.ctx._L.fhs_store_rekey(self.sk.ctx._h, self.id, None))
            return self
        eid = C.c_uint64(0)
        self.sk.ctx._check(self.sk.ctx._L.fhs_store_rekey(self.sk.ctx._h, self.id, C.byref(eid)))
        return StoredString(self.sk, eid.value)

    def select(self, query, row_chars):
        """fhs_store_select: the row named by the encrypted index `query` (MyClientKey.select_query) of this entry read as
        rows of row_chars characters -> a new StoredString of row_chars characters; this one is only read.  A
        SeededSelectQuery goes through fhs_store_select_seeded."""
        eid = C.c_uint64(0)
        ctx = self.sk.ctx
        if isinstance(query, SeededSelectQuery):
            ctx._check(ctx._L.fhs_store_select_seeded(ctx._h, self.id, int(row_chars), _ptr(query.seed), _ptr(query.bodies),
                                                      query.bits, C.byref(eid)))
            return StoredString(self.sk, eid.value)
        query = np.ascontiguousarray(query, np.uint64)
        assert query.size % SELECT_QUERY_BIT_WORDS == 0
        ctx._check(ctx._L.fhs_store_select(ctx._h, self.id, int(row_chars), _ptr(query),
                                           query.size // SELECT_QUERY_BIT_WORDS, C.byref(eid)))
        return StoredString(self.sk, eid.value)

    def select_many(self, queries, row_chars):
        """fhs_store_select_batch: one row per query (all full-form arrays, or all SeededSelectQuery) from one conversion
        launch and one CMux launch per tree level and rotate bit -> a list of new StoredStrings, in the queries' order."""
        queries = list(queries)
        n = len(queries)
        seeded = n > 0 and isinstance(queries[0], SeededSelectQuery)
        if any(isinstance(q, SeededSelectQuery) != seeded for q in queries):
            raise ValueError("select_many: the queries of one call have one form")
        if seeded:
            words = [q.bodies for q in queries]
            bits = {q.bits for q in queries}
            seeds = np.ascontiguousarray(np.stack([q.seed for q in queries]), np.uint32)
        else:
            words = [np.ascontiguousarray(q, np.uint64) for q in queries]
            assert all(w.size % SELECT_QUERY_BIT_WORDS == 0 for w in words)
            bits = {w.size // SELECT_QUERY_BIT_WORDS for w in words}
            seeds = None
        if len(bits) > 1:
            raise ValueError("select_many: the queries of one call have one bit count")
        table = (C.c_void_p * max(1, n))(*[w.ctypes.data for w in words])
        ids = (C.c_uint64 * max(1, n))()
        ctx = self.sk.ctx
        ctx._check(ctx._L.fhs_store_select_batch(ctx._h, self.id, int(row_chars), SELECT_FORM_SEEDED if seeded else SELECT_FORM_FULL,
                                                 None if seeds is None else _ptr(seeds), table, n, bits.pop() if bits else 0, ids))
        return [StoredString(self.sk, ids[i]) for i in range(n)]

    @property
    def rekeys(self):
        """fhs_store_rekey_count: re-keys inside this entry's noise (0 after an import)."""
        n = C.c_uint32(0)
        self.sk.ctx._check(self.sk.ctx._L.fhs_store_rekey_count(self.sk.ctx._h, self.id, C.byref(n)))
        return int(n.value)

    def download_packed(self, first_char=0, count=None, recipient=False):
        """fhs_store_download_packed: characters [first_char, first_char + count) straight from the parked entry as a
        PackedFheString (its first_coef = 4 first_char % 2048), under the entry's key or, recipient=True, under the key the
        loaded re-key key leads to.  Nothing is expanded; needs no packing key; the entry stays as it is."""
        if count is None:
            count = len(self) - first_char
        p = PackedFheString.empty(max(0, int(count)), store_packed_words(first_char, max(0, int(count)))[2])
        self.sk.ctx._check(self.sk.ctx._L.fhs_store_download_packed(self.sk.ctx._h, self.id, int(first_char), int(count),
                                                                    int(bool(recipient)), _ptr(p.mask16), _ptr(p.body16)))
        return p

    def export(self):
        """fhs_store_export -> (CompactFheString, meta[4n] u64); store_export_to_bytes serialises the pair."""
        n = len(self)
        c = CompactFheString(n, np.zeros(((4 * n + 2047) // 2048, 2048), np.uint32), np.zeros(4 * n, np.uint32))
        meta = np.zeros(4 * n, np.uint64)
        self.sk.ctx._check(self.sk.ctx._L.fhs_store_export(self.sk.ctx._h, self.id, _ptr(c.mask32), _ptr(c.body32), _ptr(meta)))
        return c, meta


def expand_compressed_server_key(seed, bsk_bodies, ksk_bodies):
    """fhs_expand_compressed_server_key: host expansion to the standard-domain (bsk, ksk) of fhs_load_server_key."""
    seed = np.ascontiguousarray(seed, np.uint32)
    bsk_bodies = np.ascontiguousarray(bsk_bodies, np.uint64)
    ksk_bodies = np.ascontiguousarray(ksk_bodies, np.uint64)
    assert seed.size == 8 and bsk_bodies.size == 742 * 2 * 2048 and ksk_bodies.size == 2048 * 5
    bsk = np.empty(742 * 4 * 2048, np.uint64)
    ksk = np.empty(2048 * 5 * 743, np.uint64)
    if lib().fhs_expand_compressed_server_key(_ptr(seed), _ptr(bsk_bodies), _ptr(ksk_bodies), _ptr(bsk), _ptr(ksk)) != 0:
        raise FhsError("fhs_expand_compressed_server_key failed")
    return bsk, ksk


class FheSplit:
    """Vec<FheString> + pattern_found (src/ciphertext/fhesplit.rs:5-8)."""

    def __init__(self, buffers, pattern_found):
        self.buffers = buffers
        self.pattern_found = pattern_found

    @staticmethod
    def decrypt(fhe_split, my_client_key):                               # fhesplit.rs:29-40
        return ([my_client_key.decrypt(b) for b in fhe_split.buffers],
                my_client_key.decrypt_char(fhe_split.pattern_found))


def trim_vector(vec):
    """src/utils.rs:59-92."""
    vec = list(vec)
    while vec and vec[0] == "":
        vec.pop(0)
    while vec and vec[-1] == "":
        vec.pop()
    return vec


def _harr(chars):
    arr = (C.c_uint64 * max(1, len(chars)))()
    for i, ch in enumerate(chars):
        arr[i] = ch.h
    return arr


class MyServerKey:
    """MyServerKey (src/server_key/mod.rs:13-16) on one MI355X."""

    device_resident = True   # ciphertexts live in HBM; export/import take device pointers

    def __init__(self, ctx):
        self.ctx = ctx
        self._stats = None

    @classmethod
    def from_client_key(cls, client_key, device_id=0, arith=0):
        ctx = Context(device_id)
        ctx.set_arithmetic(arith)
        ctx.load_server_key(client_key.bsk(), client_key.ksk())
        if arith in (2, 3):
            ctx.load_multibit_key(client_key.bsk_mb2())
        return cls(ctx)

    @classmethod
    def planner(cls):
        """Planner context (no GPU): DAG statistics of any op -- PBS count, levels, level widths, noise bookkeeping."""
        return cls(Context(planner=True))

    def dummy_string(self, n):
        """n placeholder chars for a planner context (contents are never read)."""
        z = np.zeros((4, BIG_CT), np.uint64)
        return FheString([self.upload_char(z) for _ in range(n)])

    @classmethod
    def from_key_file(cls, path, device_id=0, arith=0, multibit_key_path=None):
        ctx = Context(device_id)
        ctx.set_arithmetic(arith)
        ctx._check(ctx._L.fhs_load_server_key_file(ctx._h, str(path).encode()))
        if multibit_key_path is not None:                      # kind 3 file, needed by arithmetics 2 and 3
            ctx._check(ctx._L.fhs_load_multibit_key_file(ctx._h, str(multibit_key_path).encode()))
        return cls(ctx)

    @classmethod
    def from_compressed_key_file(cls, path, device_id=0, arith=0, multibit_key_path=None):
        """Kind 4 file (MyClientKey.save_compressed_server_key): the seeded masks are regenerated on the device."""
        ctx = Context(device_id)
        ctx.set_arithmetic(arith)
        ctx._check(ctx._L.fhs_load_compressed_server_key_file(ctx._h, str(path).encode()))
        if multibit_key_path is not None:
            ctx._check(ctx._L.fhs_load_multibit_key_file(ctx._h, str(multibit_key_path).encode()))
        return cls(ctx)

    @classmethod
    def from_raw_keys(cls, bsk, ksk, device_id=0, arith=0, bsk_mb2=None):
        ctx = Context(device_id)
        ctx.set_arithmetic(arith)
        ctx.load_server_key(bsk, ksk)
        if bsk_mb2 is not None:
            ctx.load_multibit_key(bsk_mb2)
        return cls(ctx)

    def close(self):
        self.ctx.close()

    def set_mode(self, mode):
        self.ctx._check(self.ctx._L.fhs_set_mode(self.ctx._h, int(mode)))

    # ---- ciphertext placement ------------------------------------------------
    def trivial(self, v):
        return FheAsciiChar(self, self.ctx._L.fhs_trivial(self.ctx._h, int(v) & 255))

    def upload_char(self, blocks):
        blocks = np.ascontiguousarray(blocks, np.uint64)
        return FheAsciiChar(self, self.ctx._L.fhs_upload(self.ctx._h, _ptr(blocks)))

    def upload_string(self, chars):
        chars = np.ascontiguousarray(chars, np.uint64).reshape(-1, 4, BIG_CT)
        n = chars.shape[0]
        hs = (C.c_uint64 * max(1, n))()
        self.ctx._check(self.ctx._L.fhs_upload_string(self.ctx._h, _ptr(chars), n, hs))
        return FheString([FheAsciiChar(self, hs[i]) for i in range(n)])

    def upload_compressed_string(self, cstr, first_char=0, count=None):
        """fhs_upload_string_compressed: characters [first_char, first_char + count) of a CompressedFheString, expanded
        on the GPU straight into this context's blocks."""
        first_char, count = cstr._window(first_char, count)
        bodies = np.ascontiguousarray(cstr.bodies[first_char:first_char + count])
        hs = (C.c_uint64 * max(1, count))()
        self.ctx._check(self.ctx._L.fhs_upload_string_compressed(self.ctx._h, _ptr(cstr.seed), _ptr(bodies), count,
                                                                 first_char, hs))
        return FheString([FheAsciiChar(self, hs[i]) for i in range(count)])

    def load_packing_key(self, key=None, path=None):
        """fhs_load_packing_key (a MyClientKey, or the words of MyClientKey.packing_key()) / fhs_load_packing_key_file
        (a kind 5 file): enables download_packed."""
        if path is not None:
            self.ctx._check(self.ctx._L.fhs_load_packing_key_file(self.ctx._h, str(path).encode()))
        else:
            self.ctx.load_packing_key(key.packing_key() if isinstance(key, MyClientKey) else key)

    def load_rekey_key(self, key=None, path=None):
        """fhs_load_rekey_key (the words of MyClientKey.rekey_key(to)) / fhs_load_rekey_key_file (a kind 7 file): enables
        StoredString.rekey and download_packed(recipient=True).  Neither: unloads the key."""
        if path is not None:
            self.ctx._check(self.ctx._L.fhs_load_rekey_key_file(self.ctx._h, str(path).encode()))
        else:
            self.ctx.load_rekey_key(key)

    def download_packed(self, fhe_string, wide=False, recipient=False):
        """fhs_download_string_packed: the string ring-packed on the GPU, 16 bits per word -> PackedFheString.
        wide=True (diagnostic) also returns the 64-bit packed GLWEs (mask64, body64) before the storage switch.
        recipient=True: fhs_download_string_packed_for, the words leave under the client key the loaded re-key key leads
        to (load_rekey_key); the 64-bit GLWEs of wide=True stay under this context's client key.  An FheU16 goes as its
        two chars, lo then hi."""
        if isinstance(fhe_string, FheU16):
            fhe_string = [fhe_string.lo, fhe_string.hi]
        chars = list(fhe_string.chars if isinstance(fhe_string, FheString) else fhe_string)
        p = PackedFheString.empty(len(chars))
        if recipient:
            mask64 = body64 = None
            if wide:
                mask64, body64 = np.zeros(p.mask16.shape, np.uint64), np.zeros(p.mask16.shape, np.uint64)
            self.ctx._check(self.ctx._L.fhs_download_string_packed_for(
                self.ctx._h, _harr(chars), len(chars), _ptr(p.mask16), _ptr(p.body16),
                None if mask64 is None else _ptr(mask64), None if body64 is None else _ptr(body64)))
            return (p, mask64, body64) if wide else p
        if not wide:
            self.ctx._check(self.ctx._L.fhs_download_string_packed(self.ctx._h, _harr(chars), len(chars), _ptr(p.mask16),
                                                                   _ptr(p.body16)))
            return p
        mask64, body64 = np.zeros(p.mask16.shape, np.uint64), np.zeros(p.mask16.shape, np.uint64)
        self.ctx._check(self.ctx._L.fhs_debug_download_string_packed64(self.ctx._h, _harr(chars), len(chars), _ptr(p.mask16),
                                                                       _ptr(p.body16), _ptr(mask64), _ptr(body64)))
        return p, mask64, body64

    def upload_compact_string(self, cstr, first_char=0, count=None):
        """fhs_upload_string_public: characters [first_char, first_char + count) of a CompactFheString, sample-extracted
        on the GPU straight into this context's blocks."""
        first_char, count = cstr._window(first_char, count)
        hs = (C.c_uint64 * max(1, count))()
        self.ctx._check(self.ctx._L.fhs_upload_string_public(self.ctx._h, _ptr(cstr.mask32), _ptr(cstr.body32), len(cstr),
                                                             first_char, count, hs))
        return FheString([FheAsciiChar(self, hs[i]) for i in range(count)])

    # ---- device-resident string store ---------------------------------------
    def store_put(self, fhe_string):
        """fhs_store_put: parks the string in HBM at 34 B per character -> StoredString.  The handles stay valid; release
        them (drop the FheString) to get the pool blocks back.  Needs the packing key."""
        chars = list(fhe_string.chars if isinstance(fhe_string, FheString) else fhe_string)
        eid = C.c_uint64(0)
        self.ctx._check(self.ctx._L.fhs_store_put(self.ctx._h, _harr(chars), len(chars), C.byref(eid)))
        return StoredString(self, eid.value)

    def store_import(self, compact, meta=None):
        """fhs_store_import: an entry from host memory (a StoredString.export(), or with meta=None a public-key encrypted
        CompactFheString parked as it arrives) -> StoredString."""
        if meta is not None:
            meta = np.ascontiguousarray(meta, np.uint64).reshape(-1)
            assert meta.size == 4 * len(compact)
        eid = C.c_uint64(0)
        self.ctx._check(self.ctx._L.fhs_store_import(self.ctx._h, _ptr(compact.mask32), _ptr(compact.body32),
                                                     None if meta is None else _ptr(meta), len(compact), C.byref(eid)))
        return StoredString(self, eid.value)

    def store_stats(self):
        """fhs_store_stats -> dict(entries, chars, device_bytes)."""
        e, n, b = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.ctx._check(self.ctx._L.fhs_store_stats(self.ctx._h, C.byref(e), C.byref(n), C.byref(b)))
        return {"entries": int(e.value), "chars": int(n.value), "device_bytes": int(b.value)}

    # ---- block pool ------------------------------------------------------------
    def pool_stats(self):
        """fhs_pool_stats -> dict(chunks, blocks_per_chunk, live, free, free_pending, device_bytes)."""
        out = (C.c_uint64 * 6)()
        self.ctx._check(self.ctx._L.fhs_pool_stats(self.ctx._h, out))
        return dict(zip(("chunks", "blocks_per_chunk", "live", "free", "free_pending", "device_bytes"), map(int, out)))

    def pool_trim(self, compact=True, keep_free_blocks=0):
        """fhs_pool_trim (not `trim`: that is the string operation of trim.rs): flush, then give back the chunks of the
        block pool that the live blocks and keep_free_blocks more do not need; compact=True first moves the live blocks
        of the emptiest chunks together on the GPU (FHS_TRIM_COMPACT), compact=False only releases chunks that are
        already empty (FHS_TRIM_RELEASE).  -> dict(blocks_moved, bytes_released)."""
        moved, released = C.c_uint64(), C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_pool_trim(self.ctx._h, TRIM_COMPACT if compact else TRIM_RELEASE,
                                                  int(keep_free_blocks), C.byref(moved), C.byref(released)))
        return {"blocks_moved": int(moved.value), "bytes_released": int(released.value)}

    def import_device(self, d_ptr):
        return FheAsciiChar(self, self.ctx._L.fhs_import_device(self.ctx._h, C.c_void_p(d_ptr)))

    def export_device(self, ch, d_ptr):
        self.flush()
        self.ctx._check(self.ctx._L.fhs_export_device(self.ctx._h, ch.h, C.c_void_p(d_ptr)))

    def export_device_async(self, ch, d_ptr):
        """Stream-ordered export (no host wait); pair with stream_handle() to order foreign work after it."""
        self.ctx._check(self.ctx._L.fhs_export_device_async(self.ctx._h, ch.h, C.c_void_p(d_ptr)))

    def stream_handle(self):
        return int(self.ctx._L.fhs_stream_handle(self.ctx._h) or 0)

    def flush(self, wait=True):
        """Run every pending PBS level.  wait=False only enqueues the launches (fhs_flush_async)."""
        if wait:
            self.ctx._check(self.ctx._L.fhs_flush(self.ctx._h))
        else:
            self.ctx._check(self.ctx._L.fhs_flush_async(self.ctx._h))

    def submit(self):
        """fhs_submit: plan what was recorded since the last submit / flush as one job (nothing runs yet)."""
        self.ctx._check(self.ctx._L.fhs_submit(self.ctx._h))

    def pump(self, n_ticks=1):
        """fhs_pump: enqueue the next n ticks (one launch group each over every job's level scheduled for it)."""
        self.ctx._check(self.ctx._L.fhs_pump(self.ctx._h, int(n_ticks)))

    def set_tick_balance(self, slots=None):
        """fhs_set_tick_balance: round-align the launch groups of fhs_submit scheduling (None = the selected kernel's
        resident slots, 0 = off)."""
        if slots is None:
            slots = self.ctx._L.fhs_resident_slots(self.ctx._h)
        self.ctx._check(self.ctx._L.fhs_set_tick_balance(self.ctx._h, int(slots)))
        return int(slots)

    def set_auto_flush(self, n_depth1):
        """fhs_set_auto_flush: peel the ready level once n_depth1 bootstraps of it are recorded (0 = off)."""
        self.ctx._check(self.ctx._L.fhs_set_auto_flush(self.ctx._h, int(n_depth1)))

    def stream_sync(self):
        self.ctx._check(self.ctx._L.fhs_stream_sync(self.ctx._h))

    def enable_level_parallel(self, rank, world, dist, torch):
        """Level-parallel multi-GPU mode inside the library (fhs_dist_level_parallel): every rank records the same
        DAG on the same ciphertexts and runs 1/world of every PBS level; one stream-ordered all-gather per level."""
        from .parallel import Dist
        if world > 1:
            self.dist = Dist.from_torch(self, dist, torch, rank, world)
            self.dist.level_parallel(True)

    def _flags(self, name, flags):
        flags = self._chars(flags)
        out = C.c_uint64()
        self.ctx._check(getattr(self.ctx._L, name)(self.ctx._h, _harr(flags), len(flags), C.byref(out)))
        return FheAsciiChar(self, out.value)

    def flags_or(self, flags): return self._flags("fhs_flags_or", flags)
    def flags_and(self, flags): return self._flags("fhs_flags_and", flags)

    def flags_first_decides(self, any_diff, verdict, tie):
        """Combine compare_partial() results of consecutive ranges: the first range that differs decides."""
        out = C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_flags_first_decides(self.ctx._h, _harr(any_diff), _harr(verdict),
                                                            len(any_diff), int(tie), C.byref(out)))
        return FheAsciiChar(self, out.value)

    def capture_pbs_inputs(self, max_rows_per_level, live=False):
        """fhs_debug_capture_pbs_inputs: sample the PBS inputs of every executed level (0 = off).  live: inside the
        ordinary execution path (rotation sharing and scheduling as in production: fhs_debug_capture_live)."""
        self.ctx._check(self.ctx._L.fhs_debug_capture_live(self.ctx._h, int(bool(live))))
        self.ctx._check(self.ctx._L.fhs_debug_capture_pbs_inputs(self.ctx._h, int(max_rows_per_level)))

    def read_capture(self):
        """-> (rows [n, 2049] u64, records: structured array level/index/lut/n_terms/sum_c2/konst/width)."""
        from ._lib import CaptureRec
        L, h = self.ctx._L, self.ctx._h
        n = C.c_size_t()
        self.ctx._check(L.fhs_debug_capture_read(h, None, None, 0, C.byref(n)))
        rows = np.zeros((n.value, BIG_CT), np.uint64)
        recs = (CaptureRec * max(1, n.value))()
        got = C.c_size_t()
        self.ctx._check(L.fhs_debug_capture_read(h, _ptr(rows), C.cast(recs, C.c_void_p), n.value, C.byref(got)))
        dt = np.dtype([("level", "u4"), ("index", "u4"), ("lut", "u4"), ("n_terms", "u4"), ("sum_c2", "i8"),
                       ("konst", "i4"), ("width", "u4")])
        return rows[:got.value], np.frombuffer(recs, dtype=dt, count=got.value).copy()

    def level_widths(self):
        """Widths of the dependency levels executed since the last stats reset (fhs_level_widths)."""
        n = C.c_size_t()
        self.ctx._check(self.ctx._L.fhs_level_widths(self.ctx._h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), np.uint32)
        self.ctx._check(self.ctx._L.fhs_level_widths(self.ctx._h, _ptr(out), n.value, C.byref(n)))
        return out[:n.value].tolist()

    def launch_groups(self):
        """Rows this rank ran in every launch group since the last stats reset (fhs_launch_groups)."""
        n = C.c_size_t()
        self.ctx._check(self.ctx._L.fhs_launch_groups(self.ctx._h, None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), np.uint32)
        self.ctx._check(self.ctx._L.fhs_launch_groups(self.ctx._h, _ptr(out), n.value, C.byref(n)))
        return out[:n.value].tolist()

    def stats(self, reset=False):
        from ._lib import Stats
        st = Stats()
        self.ctx._check(self.ctx._L.fhs_get_stats(self.ctx._h, C.byref(st)))
        out = {k: getattr(st, k) for k, _ in Stats._fields_}
        if reset:
            self.ctx._L.fhs_reset_stats(self.ctx._h)
        return out

    # ---- helpers -------------------------------------------------------------
    @staticmethod
    def _chars(x):
        return x.chars if isinstance(x, FheString) else list(x)

    def _flag_op(self, name, s, pat):
        s, pat = self._chars(s), self._chars(pat)
        out = C.c_uint64()
        rc = getattr(self.ctx._L, "fhs_str_" + name)(self.ctx._h, _harr(s), len(s), _harr(pat), len(pat),
                                                      C.byref(out))
        if rc == -4:
            raise OverflowError(self.ctx._L.fhs_last_error(self.ctx._h).decode())
        self.ctx._check(rc)
        return FheAsciiChar(self, out.value)

    def _map_op(self, name, s, n_out=None):
        s = self._chars(s)
        n_out = len(s) if n_out is None else n_out
        out = (C.c_uint64 * max(1, n_out))()
        self.ctx._check(getattr(self.ctx._L, name)(self.ctx._h, _harr(s), len(s), out))
        return FheString([FheAsciiChar(self, out[i]) for i in range(n_out)])

    # ---- the reference's methods (public_parameters accepted and ignored) -----
    def contains(self, string, needle, public_parameters=None):          # mod.rs:151
        return self._flag_op("contains", string, needle)

    def contains_clear(self, string, clear_needle, public_parameters=None):   # mod.rs:198
        s = self._chars(string)
        data = clear_needle.encode("ascii")
        out = C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_contains_clear(self.ctx._h, _harr(s), len(s), data, len(data),
                                                           C.byref(out)))
        return FheAsciiChar(self, out.value)

    def like_clear(self, string, pattern, escape=None, ignore_case=False):
        """SQL LIKE / ILIKE against a clear pattern (fhs_str_like_clear): a 0/1 flag char.  `%` any
        run of buffer characters, `_` one character that is not NUL, anything else itself; `escape` (one character) makes
        the `%`, `_` or escape character behind it a literal.  Anchored at both ends: the match ends at the end of the
        buffer or before a NUL.  pattern: str (ASCII) or bytes."""
        s = self._chars(string)
        data = pattern.encode("ascii") if isinstance(pattern, str) else bytes(pattern)
        if escape is None:
            esc = -1
        else:
            e = escape.encode("ascii") if isinstance(escape, str) else bytes(escape)
            if len(e) != 1:
                raise ValueError("escape must be one character")
            esc = e[0]
        out = C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_like_clear(self.ctx._h, _harr(s), len(s), data, len(data), esc,
                                                       _K["FHS_LIKE_IGNORE_CASE"] if ignore_case else 0, C.byref(out)))
        return FheAsciiChar(self, out.value)

    @staticmethod
    def _regex_args(pattern, ignore_case, search):
        data = pattern.encode("ascii") if isinstance(pattern, str) else bytes(pattern)
        return data, (_K["FHS_REGEX_IGNORE_CASE"] if ignore_case else 0) | (_K["FHS_REGEX_SEARCH"] if search else 0)

    def regex_clear(self, string, pattern, ignore_case=False, search=False):
        """A regular expression against a clear pattern (fhs_str_regex_clear): the 0/1 flag char of
        re.fullmatch(pattern, text, re.S) -- re.search with search=True, re.I as well with ignore_case=True -- on the text
        up to the buffer's first NUL.  The syntax is a subset of Python's bytes `re` (include/fhestring_hip.h lists it);
        what is outside it raises FhsError (FHS_ERR_ARG) and records nothing.  pattern: str (ASCII) or bytes."""
        s = self._chars(string)
        data, flags = self._regex_args(pattern, ignore_case, search)
        out = C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_regex_clear(self.ctx._h, _harr(s), len(s), data, len(data), flags, C.byref(out)))
        return FheAsciiChar(self, out.value)

    @staticmethod
    def regex_info(pattern, ignore_case=False, search=False):
        """The parser of regex_clear alone (fhs_regex_info; no context): {"code": 0, "positions": pattern positions after the
        counted repeats are expanded, "min_len": length of the shortest match}, or for a refused pattern {"code":
        FHS_ERR_ARG or FHS_ERR_LIMIT, "err_offset": byte offset of what is refused}."""
        data, flags = MyServerKey._regex_args(pattern, ignore_case, search)
        pos, low, off = C.c_size_t(), C.c_size_t(), C.c_size_t()
        rc = lib().fhs_regex_info(data, len(data), flags, C.byref(pos), C.byref(low), C.byref(off))
        if rc:
            return {"code": rc, "err_offset": off.value}
        return {"code": 0, "positions": pos.value, "min_len": low.value}

    def regex_find_clear(self, string, pattern, ignore_case=False):
        """Where the first match of a clear regular expression starts (fhs_str_regex_find_clear):
        re.search(pattern, text, re.S).start() on the text up to the buffer's first NUL, as find returns a position (255 if
        there is no match); at most 256 characters.  Syntax and errors are regex_clear's.  pattern: str (ASCII) or bytes."""
        s = self._chars(string)
        data, flags = self._regex_args(pattern, ignore_case, False)
        out = C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_regex_find_clear(self.ctx._h, _harr(s), len(s), data, len(data), flags, C.byref(out)))
        return FheAsciiChar(self, out.value)

    def regex_find_clear_wide(self, string, pattern, ignore_case=False):
        """regex_find_clear with a 16-bit position (FheU16; absent = 65535; at most 65536 characters)."""
        s = self._chars(string)
        data, flags = self._regex_args(pattern, ignore_case, False)
        lo, hi = C.c_uint64(), C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_regex_find_clear_wide(self.ctx._h, _harr(s), len(s), data, len(data), flags,
                                                                  C.byref(lo), C.byref(hi)))
        return FheU16(FheAsciiChar(self, lo.value), FheAsciiChar(self, hi.value))

    def regex_starts_clear(self, string, pattern, ignore_case=False):
        """One 0/1 flag char per buffer character (fhs_str_regex_starts_clear): 1 iff re.match(pattern, text, i) succeeds
        and no NUL stands before index i."""
        s = self._chars(string)
        data, flags = self._regex_args(pattern, ignore_case, False)
        out = (C.c_uint64 * max(1, len(s)))()
        self.ctx._check(self.ctx._L.fhs_str_regex_starts_clear(self.ctx._h, _harr(s), len(s), data, len(data), flags, out))
        return FheString([FheAsciiChar(self, out[i]) for i in range(len(s))])

    def starts_with(self, string, pattern, public_parameters=None):      # mod.rs:344
        return self._flag_op("starts_with", string, pattern)

    def ends_with(self, string, needle, public_parameters=None):         # mod.rs:241
        return self._flag_op("ends_with", string, needle)

    def find(self, string, pattern, public_parameters=None):             # mod.rs:1010
        return self._flag_op("find", string, pattern)

    def find_clear(self, string, clear_pattern, public_parameters=None):  # mod.rs:1075
        s = self._chars(string)
        data = clear_pattern.encode("ascii")
        out = C.c_uint64()
        rc = self.ctx._L.fhs_str_find_clear(self.ctx._h, _harr(s), len(s), data, len(data), C.byref(out))
        if rc == -4:
            raise OverflowError(self.ctx._L.fhs_last_error(self.ctx._h).decode())
        self.ctx._check(rc)
        return FheAsciiChar(self, out.value)

    def rfind(self, string, pattern, public_parameters=None):            # mod.rs:727
        return self._flag_op("rfind", string, pattern)

    def is_empty(self, string, public_parameters=None):                  # mod.rs:431
        s = self._chars(string)
        out = C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_is_empty(self.ctx._h, _harr(s), len(s), C.byref(out)))
        return FheAsciiChar(self, out.value)

    def len(self, string, public_parameters=None):                       # mod.rs:478
        s = self._chars(string)
        out = C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_len(self.ctx._h, _harr(s), len(s), C.byref(out)))
        return FheAsciiChar(self, out.value)

    # ---- 16-bit positions and counts (the reference's are u8: src/main.rs:20) ----
    def _wide(self, name, *args):
        lo, hi = C.c_uint64(), C.c_uint64()
        rc = getattr(self.ctx._L, name)(self.ctx._h, *args, C.byref(lo), C.byref(hi))
        if rc == -4:
            raise OverflowError(self.ctx._L.fhs_last_error(self.ctx._h).decode())
        self.ctx._check(rc)
        return FheU16(FheAsciiChar(self, lo.value), FheAsciiChar(self, hi.value))

    def find_wide(self, string, pattern):                                # mod.rs:1010, absent = WIDE_ABSENT
        s, pat = self._chars(string), self._chars(pattern)
        return self._wide("fhs_str_find_wide", _harr(s), len(s), _harr(pat), len(pat))

    def find_clear_wide(self, string, clear_pattern):                    # mod.rs:1075
        s, data = self._chars(string), clear_pattern.encode("ascii")
        return self._wide("fhs_str_find_clear_wide", _harr(s), len(s), data, len(data))

    def rfind_wide(self, string, pattern):                               # mod.rs:727
        s, pat = self._chars(string), self._chars(pattern)
        return self._wide("fhs_str_rfind_wide", _harr(s), len(s), _harr(pat), len(pat))

    def len_wide(self, string):                                          # mod.rs:478, no wrap at 256
        s = self._chars(string)
        return self._wide("fhs_str_len_wide", _harr(s), len(s))

    def count_flags_wide(self, flags):
        """The number of set flags among 0/1 flag chars (fhs_flags_count_wide)."""
        f = self._chars(flags)
        return self._wide("fhs_flags_count_wide", _harr(f), len(f))

    # ---- clear tables and classes on encrypted characters ----
    @staticmethod
    def class_set(cls):
        """The 32-byte bitmap of a character class: bytes, a set (any iterable) of ints, or a spec such as "a-zA-Z0-9_",
        with a leading ^ for the complement; x-y is a range, a - at either end and every other character itself."""
        if isinstance(cls, str):
            spec = cls.encode("latin-1")
            negate = spec.startswith(b"^")
            spec, members, i = spec[1:] if negate else spec, set(), 0
            while i < len(spec):
                if i + 2 < len(spec) and spec[i + 1] == 0x2D:
                    if spec[i + 2] < spec[i]:
                        raise ValueError("character class: range out of order in %r" % cls)
                    members.update(range(spec[i], spec[i + 2] + 1))
                    i += 3
                else:
                    members.add(spec[i])
                    i += 1
            if negate:
                members = set(range(256)) - members
        else:
            members = set(int(v) for v in cls)
            if any(v < 0 or v > 255 for v in members):
                raise ValueError("character class: members are bytes")
        bits = bytearray(32)
        for v in members:
            bits[v >> 3] |= 1 << (v & 7)
        return bytes(bits)

    def map_clear(self, string, table):
        """fhs_str_map_clear: every buffer byte x becomes table[x] (256 entries), NULs included."""
        table = bytes(table)
        if len(table) != 256:
            raise ValueError("map_clear: the table has 256 entries")
        s = self._chars(string)
        out = (C.c_uint64 * max(1, len(s)))()
        self.ctx._check(self.ctx._L.fhs_str_map_clear(self.ctx._h, _harr(s), len(s), table, out))
        return FheString([FheAsciiChar(self, out[i]) for i in range(len(s))])

    def translate(self, string, mapping):
        """bytes.translate on an encrypted string: mapping is a dict {byte: byte} (ints or one-character str / bytes) or
        a 256-byte table (bytes.maketrans).  Bytes that are not mentioned stay; 0 -> 0 unless the mapping says otherwise."""
        if isinstance(mapping, dict):
            as_int = lambda v: v if isinstance(v, int) else (v.encode("latin-1") if isinstance(v, str) else bytes(v))[0]
            table = bytearray(range(256))
            for k, v in mapping.items():
                table[as_int(k)] = as_int(v)
            mapping = bytes(table)
        return self.map_clear(string, mapping)

    def class_flags(self, string, cls):
        """fhs_str_class_flags: one 0/1 flag char per buffer character, 1 iff the byte is in the class (class_set)."""
        s = self._chars(string)
        out = (C.c_uint64 * max(1, len(s)))()
        self.ctx._check(self.ctx._L.fhs_str_class_flags(self.ctx._h, _harr(s), len(s), self.class_set(cls), out))
        return FheString([FheAsciiChar(self, out[i]) for i in range(len(s))])

    def in_class(self, char_or_string, cls):
        """A char: its 0/1 flag char; a string: the flags of its characters (class_flags)."""
        if isinstance(char_or_string, FheAsciiChar):
            return self.class_flags([char_or_string], cls)[0]
        return self.class_flags(char_or_string, cls)

    def find_class(self, string, cls):
        """Index of the first character in the class as find returns it (255 if none); at most 256 characters."""
        s = self._chars(string)
        out = C.c_uint64()
        rc = self.ctx._L.fhs_str_find_class(self.ctx._h, _harr(s), len(s), self.class_set(cls), C.byref(out))
        if rc == -4:
            raise OverflowError(self.ctx._L.fhs_last_error(self.ctx._h).decode())
        self.ctx._check(rc)
        return FheAsciiChar(self, out.value)

    def find_class_wide(self, string, cls):
        s = self._chars(string)
        return self._wide("fhs_str_find_class_wide", _harr(s), len(s), self.class_set(cls))

    def count_class(self, string, cls):
        """The number of characters in the class, 16 bits wide: class_flags + count_flags_wide."""
        return self.count_flags_wide(self.class_flags(string, cls))

    def all_in_class(self, string, cls):
        """1 iff every character of the text is in the class: the NUL padding counts as a member."""
        bits = bytearray(self.class_set(cls))
        bits[0] |= 1
        return self.flags_and(self.class_flags(string, bytes(i for i in range(256) if bits[i >> 3] >> (i & 7) & 1)))

    @staticmethod
    def user_lut(values):
        """fhs_user_lut: registers a 16-entry table (values below 32) process-wide and returns its id."""
        values = bytes(values)
        if len(values) != 16:
            raise ValueError("a user table has 16 entries")
        out = C.c_int()
        rc = lib().fhs_user_lut(values, C.byref(out))
        if rc == -4:
            raise OverflowError("the registry of user look-up tables is full")
        if rc:
            raise _coded(FhsError("fhs_user_lut: a value above 31"), rc)
        return out.value

    # ---- encrypted positions as operands (the reference only decrypts them) ----
    # `pos` is an FheAsciiChar (find, rfind, len), an FheU16 (their _wide forms) or a Python int.  The buffer is taken as
    # it is, NULs included; a position past its end -- an absent one among them -- selects nothing.  An int is plain
    # slicing with trivial NULs: no entry point, no bootstrap.
    def _pos_op(self, name, s, pos, n_out, count=None):
        wide = isinstance(pos, FheU16)
        args = [_harr(s), len(s)] + ([pos.lo.h, pos.hi.h] if wide else [pos.h]) + ([] if count is None else [count])
        outs = [(C.c_uint64 * max(1, k))() for k in n_out]
        self.ctx._check(getattr(self.ctx._L, name + ("_wide" if wide else ""))(self.ctx._h, *args, *outs))
        return [FheString([FheAsciiChar(self, o[i]) for i in range(k)]) for o, k in zip(outs, n_out)]

    def _nuls(self, k):
        return [self.trivial(0) for _ in range(k)]

    def char_at(self, string, pos):
        """buf[pos] if pos < len(buf), else NUL."""
        return self.substr(string, pos, 1)[0] if isinstance(pos, int) else \
            self._pos_op("fhs_str_char_at", self._chars(string), pos, [1])[0][0]

    def substr(self, string, start, count):
        """`count` (clear) characters from `start`: buf[start + j] if start + j < len(buf), else NUL."""
        s = self._chars(string)
        if isinstance(start, int):
            part = s[start:start + count] if 0 <= start < len(s) else []
            return FheString(part + self._nuls(count - len(part)))
        return self._pos_op("fhs_str_substr", s, start, [count], count)[0]

    def take(self, string, end):
        """The buffer with everything from `end` on set to NUL (same length)."""
        s = self._chars(string)
        if isinstance(end, int):
            end = max(0, min(end, len(s)))
            return FheString(s[:end] + self._nuls(len(s) - end))
        return self._pos_op("fhs_str_take", s, end, [len(s)])[0]

    def skip(self, string, start):
        """The buffer from `start` on, NULs behind it (same length)."""
        return self.substr(string, start, len(self._chars(string)))

    def split_at(self, string, pos):
        """(take(string, pos), skip(string, pos)); the position's bits are taken out once."""
        s = self._chars(string)
        if isinstance(pos, int):
            return self.take(s, pos), self.skip(s, pos)
        head, tail = self._pos_op("fhs_str_split_at", s, pos, [len(s), len(s)])
        return head, tail

    def slice(self, string, start, end):
        """buf[start:end] at the front of a buffer of the same length."""
        return self.skip(self.take(string, end), start)

    def eq(self, string, other, public_parameters=None):                 # mod.rs:1122
        return self._flag_op("eq", string, other)

    def ne(self, string, other, public_parameters=None):                 # mod.rs:1178
        return self._flag_op("ne", string, other)

    def eq_ignore_case(self, string, other, public_parameters=None):     # mod.rs:1221
        return self._flag_op("eq_ignore_case", string, other)

    def _compare(self, a, b, cmp):
        a, b = self._chars(a), self._chars(b)
        out = C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_compare(self.ctx._h, _harr(a), len(a), _harr(b), len(b), cmp,
                                                    C.byref(out)))
        return FheAsciiChar(self, out.value)

    def compare_partial(self, a, b, cmp):
        """(any position differs, verdict at the first differing position) of two equally long slices:
        the per-GPU partial of a position-sharded lt/le/gt/ge (cmp = 0/1/2/3)."""
        a, b = self._chars(a), self._chars(b)
        d, v = C.c_uint64(), C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_compare_partial(self.ctx._h, _harr(a), len(a), _harr(b), len(b), cmp,
                                                            C.byref(d), C.byref(v)))
        return FheAsciiChar(self, d.value), FheAsciiChar(self, v.value)

    def lt(self, a, b, public_parameters=None): return self._compare(a, b, 0)   # mod.rs:1577
    def le(self, a, b, public_parameters=None): return self._compare(a, b, 1)   # mod.rs:1613
    def gt(self, a, b, public_parameters=None): return self._compare(a, b, 2)   # mod.rs:1649
    def ge(self, a, b, public_parameters=None): return self._compare(a, b, 3)   # mod.rs:1685

    def to_upper(self, s, public_parameters=None): return self._map_op("fhs_str_to_upper", s)   # mod.rs:65
    def to_lower(self, s, public_parameters=None): return self._map_op("fhs_str_to_lower", s)   # mod.rs:110
    def trim_end(self, s, public_parameters=None): return self._map_op("fhs_str_trim_end", s)   # trim.rs:36
    def trim_start(self, s, public_parameters=None): return self._map_op("fhs_str_trim_start", s)  # trim.rs:86
    def trim(self, s, public_parameters=None): return self._map_op("fhs_str_trim", s)            # trim.rs:146
    def bubble_zeroes_right(self, s): return self._map_op("fhs_bubble_zeroes_right", s)           # utils.rs:28

    def _replace(self, s, frm, to, n=None):
        s, frm, to = self._chars(s), self._chars(frm), self._chars(to)
        cap = self.ctx._L.fhs_str_replace_len(len(s), len(frm), len(to))
        out = (C.c_uint64 * max(1, cap))()
        n_out = C.c_size_t()
        if n is None:
            rc = self.ctx._L.fhs_str_replace(self.ctx._h, _harr(s), len(s), _harr(frm), len(frm), _harr(to),
                                             len(to), out, cap, C.byref(n_out))
        else:
            rc = self.ctx._L.fhs_str_replacen(self.ctx._h, _harr(s), len(s), _harr(frm), len(frm), _harr(to),
                                              len(to), n.h, out, cap, C.byref(n_out))
        self.ctx._check(rc)
        return FheString([FheAsciiChar(self, out[i]) for i in range(n_out.value)])

    def replace(self, s, frm, to, public_parameters=None): return self._replace(s, frm, to)          # mod.rs:624
    def replacen(self, s, frm, to, n, public_parameters=None): return self._replace(s, frm, to, n)  # mod.rs:1729

    def replace_clear(self, s, clear_from, clear_to, public_parameters=None):                        # mod.rs:679
        return self._replace(s, [self.trivial(b) for b in clear_from.encode("ascii")],
                             [self.trivial(b) for b in clear_to.encode("ascii")])

    def repeat(self, s, n, public_parameters=None):                       # mod.rs:567
        s = self._chars(s)
        n_out = MAX_REPETITIONS * len(s)
        out = (C.c_uint64 * max(1, n_out))()
        self.ctx._check(self.ctx._L.fhs_str_repeat(self.ctx._h, _harr(s), len(s), n.h, out))
        return FheString([FheAsciiChar(self, out[i]) for i in range(n_out)])

    def repeat_clear(self, s, n, public_parameters=None):                 # mod.rs:517
        s = self._chars(s)
        n_out = n * len(s)
        out = (C.c_uint64 * max(1, n_out))()
        self.ctx._check(self.ctx._L.fhs_str_repeat_clear(self.ctx._h, _harr(s), len(s), n, out))
        return FheString([FheAsciiChar(self, out[i]) for i in range(n_out)])

    def concatenate(self, a, b, public_parameters=None):                  # mod.rs:1864
        a, b = self._chars(a), self._chars(b)
        out = (C.c_uint64 * max(1, len(a) + len(b)))()
        self.ctx._check(self.ctx._L.fhs_str_concatenate(self.ctx._h, _harr(a), len(a), _harr(b), len(b), out))
        return FheString([FheAsciiChar(self, out[i]) for i in range(len(a) + len(b))])

    def _strip(self, name, s, pat):
        s, pat = self._chars(s), self._chars(pat)
        out = (C.c_uint64 * max(1, len(s)))()
        found = C.c_uint64()
        self.ctx._check(getattr(self.ctx._L, name)(self.ctx._h, _harr(s), len(s), _harr(pat), len(pat), out,
                                                   C.byref(found)))
        return FheString([FheAsciiChar(self, out[i]) for i in range(len(s))]), FheAsciiChar(self, found.value)

    # ---- split family (src/server_key/split.rs) ---------------------------------
    def _split(self, kind, s, pat=(), n=None):
        s, pat = self._chars(s), self._chars(pat)
        d = self.ctx._L.fhs_str_split_dim(kind, len(s))
        out = (C.c_uint64 * max(1, d * d))()
        dim, found = C.c_size_t(), C.c_uint64()
        self.ctx._check(self.ctx._L.fhs_str_split(self.ctx._h, kind, _harr(s), len(s), _harr(pat), len(pat),
                                                  n.h if n is not None else 0, out, d * d, C.byref(dim),
                                                  C.byref(found)))
        d = dim.value
        bufs = [FheString([FheAsciiChar(self, out[i * d + j]) for j in range(d)]) for i in range(d)]
        return FheSplit(bufs, FheAsciiChar(self, found.value))

    def _clear(self, text):
        return [self.trivial(b) for b in text.encode("ascii")]

    def split(self, s, p, public_parameters=None): return self._split(0, s, p)                         # :989
    def split_clear(self, s, p, public_parameters=None): return self._split(0, s, self._clear(p))
    def split_inclusive(self, s, p, public_parameters=None): return self._split(1, s, p)               # :1020
    def split_inclusive_clear(self, s, p, public_parameters=None): return self._split(1, s, self._clear(p))
    def split_terminator(self, s, p, public_parameters=None): return self._split(2, s, p)              # :1051
    def split_terminator_clear(self, s, p, public_parameters=None): return self._split(2, s, self._clear(p))
    def splitn(self, s, p, n, public_parameters=None): return self._split(3, s, p, n)                  # :1448
    def splitn_clear(self, s, p, n, public_parameters=None): return self._split(3, s, self._clear(p), self.trivial(n))
    def rsplit(self, s, p, public_parameters=None): return self._split(4, s, p)                        # :394
    def rsplit_clear(self, s, p, public_parameters=None): return self._split(4, s, self._clear(p))
    def rsplit_terminator(self, s, p, public_parameters=None): return self._split(5, s, p)             # :504
    def rsplit_terminator_clear(self, s, p, public_parameters=None): return self._split(5, s, self._clear(p))
    def rsplitn(self, s, p, n, public_parameters=None): return self._split(6, s, p, n)                 # :421
    def rsplitn_clear(self, s, p, n, public_parameters=None): return self._split(6, s, self._clear(p), self.trivial(n))
    def rsplit_once(self, s, p, public_parameters=None): return self._split(7, s, p)                   # :462
    def rsplit_once_clear(self, s, p, public_parameters=None): return self._split(7, s, self._clear(p))
    def split_ascii_whitespace(self, s, public_parameters=None): return self._split(8, s)              # :1377

    def strip_prefix(self, s, pat, public_parameters=None): return self._strip("fhs_str_strip_prefix", s, pat)   # mod.rs:1261
    def strip_suffix(self, s, pat, public_parameters=None): return self._strip("fhs_str_strip_suffix", s, pat)   # mod.rs:1335
