/*
 * fhestring_hip.h -- C ABI of the MI355X-native TFHE backend that sits under
 * the FheString server-key operations of MakisChristou/fhestring.
 *
 * The reference has no FFI: its seam is the set of `tfhe::integer` calls made
 * from src/ciphertext/fheasciichar.rs and src/client_key.rs.
 * Every entry point below names the reference interface it replaces.  Plain
 * pointers and sizes only; every function returns 0 on success or a negative
 * error code (text via fhs_last_error); nothing unwinds across the boundary.
 *
 * Ciphertext layout (unchanged from the reference's types):
 *   block   = big LWE ciphertext, 2049 x u64 (2048 mask + body), 16 392 B
 *   char    = FheAsciiChar = 4 blocks, little-endian 2-bit digits, 65 568 B
 *             (src/ciphertext/fheasciichar.rs:8-10)
 *   string  = contiguous array of chars (src/ciphertext/fhestring.rs:6-9)
 * Keys: PARAM_MESSAGE_2_CARRY_2_KS_PBS (src/main.rs:3,43)
 *   bsk[742][2][2][2048] u64  standard-domain GGSW rows (row 0 mask, row 1 body)
 *   ksk[2048][5][743]    u64
 */
#ifndef FHESTRING_HIP_H
#define FHESTRING_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHS_LWE_N 742
#define FHS_POLY_N 2048
#define FHS_BIG_CT 2049          /* u64 words per block */
#define FHS_SMALL_CT 743
#define FHS_BLOCKS_PER_CHAR 4    /* MAX_BLOCKS, src/main.rs:23 */
#define FHS_CHAR_WORDS (4 * 2049)
#define FHS_BSK_WORDS ((size_t)742 * 4 * 2048)
#define FHS_KSK_WORDS ((size_t)2048 * 5 * 743)
#define FHS_MAX_FIND_LENGTH 255  /* src/main.rs:20 */
#define FHS_MAX_REPETITIONS 16   /* src/main.rs:17 */
#define FHS_MAX_FIND_LENGTH_WIDE 65535  /* the limit of the _wide forms, where the reference has 255 (src/main.rs:20) */
#define FHS_WIDE_ABSENT 65535           /* "not found" of the _wide forms, where the reference has 255 (mod.rs:1023) */

#define FHS_OK 0
#define FHS_ERR_ARG (-1)
#define FHS_ERR_HIP (-2)
#define FHS_ERR_STATE (-3)
#define FHS_ERR_LIMIT (-4)       /* the reference's panic!("Maximum supported size for find reached") */

typedef struct fhs_ctx fhs_ctx;
typedef struct fhs_client fhs_client;
typedef uint64_t fhs_char_t;     /* opaque handle of one lazily evaluated FheAsciiChar */

/* ---- context / server key -------------------------------------------------
 * replaces: tfhe::integer::ServerKey held by MyServerKey (src/server_key/mod.rs:13-16) */
int fhs_ctx_create(int device_id, fhs_ctx **out);
/* Planner context: no device, no key.  Every fhs_* op records its DAG exactly as on a real context and fhs_flush
 * levelises it, so the statistics (PBS count, dependency levels and their widths, noise bookkeeping) are those of the
 * real run -- but NOTHING is computed: fhs_download / exports / raw PBS entry points fail with FHS_ERR_STATE.  Host logic
 * only (capacity planning, the CPU test-suite's checks of DAG shape and noise budget); not a CPU fallback. */
int fhs_ctx_create_planner(fhs_ctx **out);
void fhs_ctx_destroy(fhs_ctx *ctx);
const char *fhs_last_error(const fhs_ctx *ctx);
/* Copies the key to the device; the BSK is rounded to the 58-bit torus grid and
 * transformed to the device NTT representation (DESIGN.md "BSK precision"). */
int fhs_load_server_key(fhs_ctx *ctx, const uint64_t *bsk, const uint64_t *ksk);
/* Arithmetic of the negacyclic products inside blind rotation.  EXACT_NTT (default): exact integer
 * arithmetic over two 47-bit NTT primes.  F64_FFT: folded f64 complex FFT, the algorithm class of the
 * reference's CPU engine (tfhe 0.5.2 + concrete-fft 0.4.0, Cargo.lock:168-179) - ~3x faster, approximate
 * at the 2^-53 relative level (far below the scheme's noise) and deterministic.  fhs_set_arithmetic and
 * fhs_load_server_key may come in either order: the standard-domain key stays on the device (48.6 MB) and its
 * Fourier-domain form is built at the key load when F64_FFT is already selected, otherwise the first time it is
 * selected (round 5; before that a key loaded first left a drop-in host on the 3.7x slower exact path).  Switching
 * back and forth is always allowed. */
#define FHS_ARITH_EXACT_NTT 0
#define FHS_ARITH_F64_FFT 1
/* F64_FFT_MB2: the f64 FFT arithmetic with TWO LWE key bits per GGSW x GLWE external product (371 products per bootstrap
 * instead of 742; the "multi-bit" blind rotation of Joye-Paillier / tfhe-rs' GPU backend at group size 2, here on the
 * reference's own parameter set: dimensions, bases, noise distributions and keyswitch unchanged).  Needs the pair key
 * (three GGSWs per pair of key bits, fhs_client_bsk_mb2) loaded with fhs_load_multibit_key AFTER fhs_load_server_key in
 * arithmetic 1 or 2.  Same inputs, same outputs up to noise (bootstrap output sigma 2^49.62 instead of 2^48.87; the
 * string layer's noise margins hold in this arithmetic too, tests/test_gpu_noise.py), bit-exact against mode 4 of the
 * CPU oracle.  csrc/fftmb_kernels.hip. */
#define FHS_ARITH_F64_FFT_MB2 2
/* EXACT_NTT_MB2: the same two-key-bits-per-product blind rotation in EXACT integer arithmetic (two-prime NTT, like
 * EXACT_NTT): no f64 rounding anywhere, bootstrap output sigma 2^48.8 (lower than the classic f64 FFT's), 1.6x the rate
 * of EXACT_NTT.  Working order: fhs_load_server_key, then fhs_load_multibit_key WHILE arithmetic 0 (EXACT_NTT) is
 * selected -- the pair key is converted for the arithmetic selected at that moment: residues modulo the two NTT primes
 * on the 57-bit torus grid for 0 / 3, the Fourier domain for 1 / 2 -- then fhs_set_arithmetic(3), which is refused
 * until the converted key exists (likewise: load under arithmetic 1, then select 2).
 * Bit-exact against mode 5 of the CPU oracle (an independent exact algorithm).  csrc/nttmb_kernels.hip. */
#define FHS_ARITH_EXACT_NTT_MB2 3
#define FHS_BSK_MB2_WORDS ((size_t)371 * 3 * 4 * 2048)
int fhs_load_multibit_key(fhs_ctx *ctx, const uint64_t *bsk_mb2 /*[371][3][2 rows][2 cols][2048]*/);
int fhs_set_arithmetic(fhs_ctx *ctx, int arith);
int fhs_get_arithmetic(const fhs_ctx *ctx);
/* Tuning knob of the F64_FFT arithmetic: batches of at most `max_batch` ciphertexts run on the 4-wavefront kernel
 * (lower latency), larger ones on the 2-wavefront kernel (higher throughput).  Default 512; 0 = never, a huge value
 * = always.  Both kernels produce identical bits. */
int fhs_set_fft4_max_batch(fhs_ctx *ctx, int max_batch);
/* Tuning knob: a blind-rotation launch of arithmetic `arith` is cut into chunks of n_ciphertexts (0 = the whole batch in
 * one launch).  Every chunk starts all workgroups on the first key element together again, which keeps the key stream
 * inside the L2 for the kernels whose key does not fit it otherwise.  Results are identical. */
int fhs_set_launch_chunk(fhs_ctx *ctx, int arith, size_t n_ciphertexts);
/* Diagnostic: the host-derived twiddle tables of the F64_FFT mode (W[1024] re/im; U[16] re/im, 3 used). */
void fhs_fft_tables(double *w_re, double *w_im, double *u_re, double *u_im);
/* ... and the monomial evaluation table of the F64_FFT_MB2 mode: exp(i*pi*k/2048), k < 4096, (re, im) pairs. */
void fhs_fft_mono_table(double *mono /*[4096][2]*/);

/* ---- raw batched PBS (the hot path; kernel-level parity tests use these) ----
 * replaces: tfhe::shortint::ServerKey::apply_lookup_table on B blocks.
 * in[B][2049], lut_idx[B], luts[L][2048] (LUT body polynomials), out[B][2049]: host memory. */
int fhs_pbs_batch(fhs_ctx *ctx, const uint64_t *in, const uint32_t *lut_idx, const uint64_t *luts,
                  size_t n_luts, uint64_t *out, size_t B);
/* keyswitch + modulus switch only: ms_out[B][743] values in [0,4096) */
int fhs_keyswitch_modswitch_batch(fhs_ctx *ctx, const uint64_t *in, uint32_t *ms_out, size_t B);
/* Rotation sharing at the raw boundary: ONE keyswitch + blind rotation per input and n_shifts sample extractions of its
 * accumulator: out[b][s] ([B][n_shifts][2049]) is what a bootstrap of (in[b] + shifts[b][s] * 2^59) with the same table
 * yields (shifts in message units, 0..31; 0 = fhs_pbs_batch's output): adding c * 2^59 to a body moves the modulus-switched
 * body by exactly 128 c, i.e. rotates the accumulator by X^(128 c), so coefficient 128 c of ONE accumulator is the other
 * bootstrap's coefficient 0.  The string layer gets this automatically: rows of one dependency level that apply the same
 * table to the same linear combination up to its trivial constant -- the nibble of a character tested against the nibbles
 * of a clear pattern, is0(x - c) -- share a rotation (fhs_set_rotation_sharing, on by default in fused mode;
 * fhs_stats.pbs_extracted counts them).  shortint::ServerKey::apply_lookup_table per shifted input, batched. */
int fhs_pbs_batch_shifted(fhs_ctx *ctx, const uint64_t *in, const uint32_t *lut_idx, const uint64_t *luts, size_t n_luts,
                          const uint32_t *shifts /*[B][n_shifts]*/, size_t n_shifts, uint64_t *out, size_t B);
int fhs_set_rotation_sharing(fhs_ctx *ctx, int on);
/* Kernel-level tests: blind rotation + sample extraction only, in the selected arithmetic, from GIVEN keyswitched LWEs
 * ks[B][743] (u64 torus; the kernels apply the modulus switch to 2N = 4096 themselves) -> out[B][2049]. */
int fhs_debug_blind_rotate_batch(fhs_ctx *ctx, const uint64_t *ks, const uint32_t *lut_idx, const uint64_t *luts,
                                 size_t n_luts, uint64_t *out, size_t B);
/* Device-resident variant: all pointers are device pointers (e.g. torch tensors' data_ptr); work is enqueued
 * on `hip_stream` (0 = default).  A context owns one set of scratch buffers and one work counter: calls on it
 * must be ordered (one stream at a time); use several contexts for concurrent streams. */
int fhs_pbs_batch_device(fhs_ctx *ctx, const uint64_t *d_in, const uint32_t *d_lut_idx,
                         const uint64_t *d_luts, uint64_t *d_out, size_t B, void *hip_stream);
/* Average duration (ms) of the blind-rotation / keyswitch KERNEL launches since the last reset, measured with HIP events
 * on the launch stream, and the number of kernel launches timed (a batch cut into one-round launches --
 * fhs_set_launch_chunk, the default of the f64 kernels -- counts every launch: the figure is what `rocprofv3
 * --kernel-trace --stats` reports per kernel; x launches = the time of the batches). */
int fhs_kernel_timing(fhs_ctx *ctx, int reset, double *blind_rotate_ms, double *keyswitch_ms,
                      uint64_t *n_blind_rotate, uint64_t *n_keyswitch, uint64_t *pbs_in_launches);
/* Per kernel class: kind 0 = blind rotation on the exact-NTT kernel or the 2-wavefront FFT kernel (fhs_kernel_timing
 * reports this one), 1 = keyswitch, 2 = blind rotation on the 4-wavefront FFT kernel (batches <= fft4_max_batch),
 * 3 = those launches of kind 0 that ran the shifted-accumulator instantiation of the 2-wavefront FFT kernel: every look-up
 * table of the launch had the low 8 bits of all its words clear (the catalogue and user tables; looked at once, when a
 * table array is uploaded).  Tables behind a caller's device pointer and tables with other words run the general
 * instantiation, with the same result.  Does not reset. */
int fhs_kernel_timing_kind(fhs_ctx *ctx, int kind, double *avg_ms, uint64_t *launches, uint64_t *pbs_in_launches);

/* ---- FheAsciiChar boundary ops (lazy DAG nodes) ------------------------------
 * Each constructor mirrors one method of src/ciphertext/fheasciichar.rs and returns a
 * handle; nothing runs until fhs_flush / fhs_download. 0 is never a valid handle. */
fhs_char_t fhs_trivial(fhs_ctx *ctx, uint8_t value);                    /* encrypt_trivial :17-25 */
fhs_char_t fhs_upload(fhs_ctx *ctx, const uint64_t *blocks /*[4][2049]*/); /* FheAsciiChar::new :13 */
/* n characters back to back ([n][4][2049] words, FheString.bytes of fhestring.rs:6-9 as the client produced them): one
 * staged copy and one scatter launch instead of one pageable copy per block (a 64-character string: 0.5 ms
 * instead of 2.5 ms).  out[n] receives the handles. */
int fhs_upload_string(fhs_ctx *ctx, const uint64_t *blocks, size_t n, fhs_char_t *out);
fhs_char_t fhs_eq(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);            /* eq  :35-38 */
fhs_char_t fhs_ne(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);            /* ne  :40-43 */
fhs_char_t fhs_le(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);            /* le  :45-48 */
fhs_char_t fhs_lt(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);            /* lt  :50-53 */
fhs_char_t fhs_ge(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);            /* ge  :55-58 */
fhs_char_t fhs_gt(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);            /* gt  :60-63 */
fhs_char_t fhs_bitand(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);        /* bitand :65-72 */
fhs_char_t fhs_bitor(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);         /* bitor  :74-81 */
fhs_char_t fhs_sub(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);           /* sub :83-86 */
fhs_char_t fhs_add(fhs_ctx *ctx, fhs_char_t a, fhs_char_t b);           /* add :88-91 */
fhs_char_t fhs_if_then_else(fhs_ctx *ctx, fhs_char_t cond, fhs_char_t t, fhs_char_t f); /* :93-104 */
fhs_char_t fhs_flip(fhs_ctx *ctx, fhs_char_t a);                        /* flip :161-168 */
fhs_char_t fhs_is_whitespace(fhs_ctx *ctx, fhs_char_t a);               /* :106-130 */
fhs_char_t fhs_is_uppercase(fhs_ctx *ctx, fhs_char_t a);                /* :132-144 */
fhs_char_t fhs_is_lowercase(fhs_ctx *ctx, fhs_char_t a);                /* :146-158 */
fhs_char_t fhs_clone(fhs_ctx *ctx, fhs_char_t a);                       /* #[derive(Clone)] :7 */
int fhs_release(fhs_ctx *ctx, fhs_char_t a);
int fhs_flush(fhs_ctx *ctx);                                             /* run every pending level */
/* Same, but only enqueues the launches on the context's HIP stream and returns (fhs_stream_sync, a download
 * or the next fhs_flush waits).  Lets several contexts on one GPU overlap: the narrow tail levels of one
 * operation run beside the wide first level of the next (bench.py --pipelines). */
int fhs_flush_async(fhs_ctx *ctx);
/* Level-skewed batching of independent requests (a server's steady state).  fhs_submit plans everything recorded since
 * the last submit / flush as one JOB and schedules its dependency levels on consecutive TICKS; fhs_pump(ctx, n) enqueues
 * the next n ticks, each as ONE launch group over the union of every job's level scheduled for it.  With one submit + one
 * pump per request, the narrow tail levels of request k ride in the wide launch of request k + 1 (a 64-char contains has
 * levels 496 / 62 / 5 / 1 wide: alone, the last three pay one bootstrap latency each on an almost empty GPU).  A job
 * that consumes results of an unfinished job is scheduled behind it.  Results are complete after fhs_flush (which
 * drains every tick) or a download. */
int fhs_submit(fhs_ctx *ctx);
/* Automatic partial flush: once `n_pending` bootstraps whose inputs are all available (dependency depth 1) are recorded,
 * that level is planned and enqueued while the caller keeps recording the rest of the operation; the other pending
 * bootstraps stay pending, one level shallower (default 8192; 0 = off).  On a device the level is also peeled as soon as
 * a grid's worth (1024) is ready and the previous launch group has finished.  Hides the host time of building large
 * DAGs (a 1024-character replace records 256 k bootstraps) behind GPU work.  Contexts driven with fhs_submit never
 * flush on their own. */
int fhs_set_auto_flush(fhs_ctx *ctx, size_t n_pending);
int fhs_pump(fhs_ctx *ctx, size_t n_ticks);
/* Round alignment of the launch groups (fhs_submit scheduling): the persistent blind-rotation kernel works on `slots`
 * ciphertexts at a time (fhs_resident_slots: 1024 on an MI355X for the f64-FFT kernels), so a launch group of 3.5 x slots
 * rows leaves half the chip idle during its last round.  With balancing on, a job level that would leave its tick's
 * group with a partly filled last round keeps only the rows that fill whole rounds; the excess (less than one round)
 * runs one tick later together with everything that consumes it.  Results are unchanged; a few results of a request are
 * complete one tick later.  0 = off (default). */
int fhs_set_tick_balance(fhs_ctx *ctx, size_t slots);
int fhs_resident_slots(const fhs_ctx *ctx);
int fhs_download(fhs_ctx *ctx, fhs_char_t a, uint64_t *blocks /*[4][2049]*/);
/* device-to-device import/export of one char (multi-GPU gather of partial results) */
/* n characters at once into [n][4][2049] words (what MyClientKey::decrypt, src/client_key.rs:89-106, walks): one gather
 * launch and one copy per 2048 blocks instead of a synchronous 16 KB copy per block (a 1025-character replace result:
 * ~10 ms instead of ~120 ms). */
int fhs_download_string(fhs_ctx *ctx, const fhs_char_t *chars, size_t n, uint64_t *blocks);
int fhs_export_device(fhs_ctx *ctx, fhs_char_t a, uint64_t *d_blocks /*[4][2049] device*/);
/* Stream-ordered variant: flushes asynchronously and enqueues the copies on the context's stream, no host wait.
 * fhs_stream_handle returns that hipStream_t so a caller can order its own work (e.g. an RCCL all-gather issued
 * under torch.cuda.ExternalStream) after the export and before a following fhs_import_device. */
int fhs_export_device_async(fhs_ctx *ctx, fhs_char_t a, uint64_t *d_blocks /*[4][2049] device*/);
void *fhs_stream_handle(fhs_ctx *ctx);
/* One char from device memory, d_blocks[4][2049] in the layout of fhs_export_device; the handle enters the noise
 * bookkeeping at figure 1 like an upload (fhs_char_set_noise declares more).  The four copies are only ENQUEUED on the
 * context's stream (fhs_stream_handle) when the call returns:
 *  - the source must be complete before the call: the caller orders its producer in front of the copy, e.g. records an
 *    event behind the producer and makes the stream of fhs_stream_handle wait on it, or waits on the host;
 *  - the source must stay unchanged until that stream has passed the copy: after fhs_stream_sync (or any call that
 *    waits for the stream, such as a download of the handle), or behind an event recorded on that stream after the call. */
fhs_char_t fhs_import_device(fhs_ctx *ctx, const uint64_t *d_blocks);

/* ---- MyServerKey string methods (src/server_key/mod.rs, trim.rs) --------------
 * Strings are arrays of handles (FheString.bytes). mode: 0 = as written in the reference
 * (same op sequence), 1 = re-associated (log-depth trees, single-block flags; decrypts
 * identically).  Outputs are fresh handles owned by the caller. */
#define FHS_MODE_AS_WRITTEN 0
#define FHS_MODE_FUSED 1
int fhs_set_mode(fhs_ctx *ctx, int mode);
int fhs_str_contains(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out);      /* mod.rs:151 */
int fhs_str_contains_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, fhs_char_t *out);      /* mod.rs:198 */
int fhs_str_starts_with(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out);   /* mod.rs:344 */
int fhs_str_ends_with(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out);     /* mod.rs:241 */
int fhs_str_find(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out);          /* mod.rs:1010 */
int fhs_str_find_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, fhs_char_t *out);          /* mod.rs:1075 */
int fhs_str_rfind(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out);         /* mod.rs:727 */
int fhs_str_is_empty(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out);                                       /* mod.rs:431 */
int fhs_str_len(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out);                                            /* mod.rs:478 */
int fhs_str_eq(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, fhs_char_t *out);            /* mod.rs:1122 */
int fhs_str_ne(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, fhs_char_t *out);            /* mod.rs:1178 */
int fhs_str_eq_ignore_case(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, fhs_char_t *out);/* mod.rs:1221 */
/* cmp: 0 lt, 1 le, 2 gt, 3 ge (enum Comparison, fhestring.rs:11-16) */
int fhs_str_compare(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, int cmp, fhs_char_t *out); /* mod.rs:1470 */
/* Positional half of the comparison (mod.rs:1497-1518) on two slices of equal length n: *any_diff = some position
 * differs, *verdict = a[i] < b[i] (cmp 0,1) resp. a[i] > b[i] (cmp 2,3) at the FIRST differing position, 0 if none.
 * Per-GPU partial of a position-sharded comparison: the first range that differs decides. */
int fhs_str_compare_partial(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, int cmp,
                            fhs_char_t *any_diff, fhs_char_t *verdict);
int fhs_str_to_upper(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out /*[n]*/);                               /* mod.rs:65 */
int fhs_str_to_lower(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out /*[n]*/);                               /* mod.rs:110 */
/* out_cap >= fhs_str_replace_len(n, m_from, m_to); *out_len receives the produced length */
size_t fhs_str_replace_len(size_t n, size_t m_from, size_t m_to);
int fhs_str_replace(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *from, size_t mf,
                    const fhs_char_t *to, size_t mt, fhs_char_t *out, size_t out_cap, size_t *out_len);                 /* mod.rs:624 */
int fhs_str_replacen(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *from, size_t mf,
                     const fhs_char_t *to, size_t mt, fhs_char_t count, fhs_char_t *out, size_t out_cap, size_t *out_len); /* mod.rs:1729 */
int fhs_str_repeat(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t count, fhs_char_t *out /*[16*n]*/);             /* mod.rs:567 */
int fhs_str_repeat_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, size_t count, fhs_char_t *out /*[count*n]*/);        /* mod.rs:517 */
int fhs_str_concatenate(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, fhs_char_t *out /*[na+nb]*/); /* mod.rs:1864 */
int fhs_str_strip_prefix(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out /*[n]*/, fhs_char_t *found); /* mod.rs:1261 */
int fhs_str_strip_suffix(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out /*[n]*/, fhs_char_t *found); /* mod.rs:1335 */
int fhs_str_trim_end(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out /*[n]*/);                               /* trim.rs:36 */
int fhs_str_trim_start(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out /*[n]*/);                             /* trim.rs:86 */
int fhs_str_trim(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out /*[n]*/);                                   /* trim.rs:146 */
int fhs_bubble_zeroes_right(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out /*[n]*/);                        /* utils.rs:28 */
/* split family (src/server_key/split.rs, FheSplit of src/ciphertext/fhesplit.rs:5-8).
 * kind: 0 split :989, 1 split_inclusive :1020, 2 split_terminator :1051, 3 splitn :1448, 4 rsplit :394,
 * 5 rsplit_terminator :504, 6 rsplitn :421, 7 rsplit_once :462, 8 split_ascii_whitespace :1377.
 * `count` is the encrypted (or trivial) n of splitn/rsplitn, 0 otherwise.  The reference returns
 * d buffers of d chars with d = n + 1 (d = n for kind 8): out[d*d] row-major, *dim = d. */
size_t fhs_str_split_dim(int kind, size_t n);
int fhs_str_split(fhs_ctx *c, int kind, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m,
                  fhs_char_t count, fhs_char_t *out, size_t out_cap, size_t *dim, fhs_char_t *found);
/* OR / AND of n 0/1 flag chars in log_15(n) levels (chains of bitor/bitand :65-81 re-associated);
 * used to combine per-GPU partial results after the gather. */
int fhs_flags_or(fhs_ctx *c, const fhs_char_t *flags, size_t n, fhs_char_t *out);
int fhs_flags_and(fhs_ctx *c, const fhs_char_t *flags, size_t n, fhs_char_t *out);
/* Combines the partials of fhs_str_compare_partial over n consecutive ranges (string order): the first range that
 * differs decides; `tie` (0 or 1) if none differs. */
int fhs_flags_first_decides(fhs_ctx *c, const fhs_char_t *any_diff, const fhs_char_t *verdict, size_t n, int tie,
                            fhs_char_t *out);

/* ---- wide positions and counts -------------------------------------------------------------------------------
 * The reference's positions and lengths are u8 (MAX_FIND_LENGTH, src/main.rs:20): find / rfind panic from 255 + m
 * characters on, len wraps modulo 256.  The _wide forms return a 16-bit unsigned value as TWO ordinary chars,
 * value = *lo + 256 * *hi (eight little-endian base-4 digits; download, packed download, store, fhs_char_sum_c2,
 * fhs_trivial_value and the char operators take either half like any char).  Same loops, same quirks, both modes;
 * "not found" is FHS_WIDE_ABSENT; FHS_ERR_LIMIT once the string (with the NUL that rfind pushes) has
 * FHS_MAX_FIND_LENGTH_WIDE + m characters, checked before anything is recorded.  The u8 entry points are unchanged. */
int fhs_str_find_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *lo, fhs_char_t *hi);       /* mod.rs:1010-1053, widens :1023-1027 and :1044 */
int fhs_str_find_clear_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, fhs_char_t *lo, fhs_char_t *hi);       /* mod.rs:1075, widens :1023-1027 and :1044 */
int fhs_str_rfind_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *lo, fhs_char_t *hi);      /* mod.rs:727-790, widens :739-744, :753 and :783 */
int fhs_str_len_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *lo, fhs_char_t *hi);                                         /* mod.rs:478-493, widens the u8 counter of :485-490 */
/* The number of set flags among n 0/1 flag chars -- the rows of a scanned table that matched, say: 256 of them already
 * overflow a char (the u8 adds of fheasciichar.rs:88-91 chained as in mod.rs:485-490, with a carry into *hi). */
int fhs_flags_count_wide(fhs_ctx *c, const fhs_char_t *flags, size_t n, fhs_char_t *lo, fhs_char_t *hi);

/* ---- encrypted positions as operands -------------------------------------------------------------------------
 * What find / rfind / len and their _wide forms return can be used on the server (the reference only ever decrypts
 * it).  With buf the n characters of s as byte values, NULs included (nothing is compacted), and p the value of the
 * position -- one char, or pos_lo + 256 * pos_hi:
 *   char_at   *out = buf[p] if p < n, else 0
 *   substr    out[j] = buf[p + j] if p + j < n, else 0, for j < count (count is clear)
 *   take      out[j] = buf[j] if j < p, else 0, for j < n
 *   split_at  head = take(s, p), tail = substr(s, p, n)
 * p is taken literally: a u8 255 on 300 characters is index 255.  An absent position (255 on n <= 255,
 * FHS_WIDE_ABSENT) is past the end: substr and char_at give NULs, take the whole buffer, split_at (s, "").  On a string
 * of text followed by NUL padding these are text[p:p+count], text[:p] and text[p:].  Both modes; no length limit.
 * n == 0 gives trivial NULs and count == 0 nothing, with nothing recorded. */
int fhs_str_char_at(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos, fhs_char_t *out);
int fhs_str_char_at_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos_lo, fhs_char_t pos_hi, fhs_char_t *out);
int fhs_str_substr(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos, size_t count, fhs_char_t *out /*[count]*/);
int fhs_str_substr_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos_lo, fhs_char_t pos_hi, size_t count, fhs_char_t *out /*[count]*/);
int fhs_str_take(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos, fhs_char_t *out /*[n]*/);
int fhs_str_take_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos_lo, fhs_char_t pos_hi, fhs_char_t *out /*[n]*/);
int fhs_str_split_at(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos, fhs_char_t *head /*[n]*/, fhs_char_t *tail /*[n]*/);
int fhs_str_split_at_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos_lo, fhs_char_t pos_hi, fhs_char_t *head /*[n]*/, fhs_char_t *tail /*[n]*/);

/* ---- LIKE against a clear pattern ----------------------------------------------------------------------------
 * SQL LIKE / ILIKE on the n characters of s (the reference has no such method); *out is a 0/1 flag char.  In the m
 * bytes of pat, '%' matches any run of buffer characters (none included, NULs included), '_' exactly one character
 * that is not NUL, any other byte itself; with an escape byte e the pairs e%, e_ and ee are the literals %, _ and e.
 * The match starts at index 0 and must end at an index j with j == n or buf[j] == 0: on text followed by NUL padding
 * (what every method here produces) this is SQL LIKE on the text; on any buffer it is Python's
 *   re.match(rb'\A' + body + rb'(?=\x00|\Z)', buf, re.S)
 * with body = [\x00-\xff]* for '%', [^\x00] for '_' and the escaped byte for a literal.  FHS_LIKE_IGNORE_CASE folds
 * the ASCII letters of the pattern (re.I).  An empty pattern matches the empty string only, a pattern of '%' alone
 * everything, and a pattern with more tokens other than '%' than n nothing: the last two record nothing.  Both modes;
 * no length limit.  FHS_ERR_ARG, before anything is recorded: a NUL in pat, an escape byte that is 0, '%' or '_', an
 * escape at the end of pat or before anything but '%', '_' or itself, unknown flag bits, a null out. */
#define FHS_LIKE_IGNORE_CASE 1
int fhs_str_like_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, int escape /* -1: none, else 1..255 */,
                       uint32_t flags, fhs_char_t *out);

/* ---- regular expressions against a clear pattern ---------------------------------------
 * With text = the n characters of s up to the first NUL (all of them if there is none), *out is the 0/1 flag char of
 *   re.fullmatch(pat, text, re.S)                    Python, bytes; re.I as well with FHS_REGEX_IGNORE_CASE
 *   re.search(pat, text, re.S)                       with FHS_REGEX_SEARCH: the same engine on .*(?:pat).*
 * No atom ever matches NUL ('.', negated classes and \D \W \S exclude it), so on the buffer the condition is: the match
 * starts at index 0, uses atoms only, and ends at j with j == n or buf[j] == 0 -- LIKE's end anchor.  n == 0 is allowed.
 * The syntax is a strict subset of Python's bytes `re`:
 *   literal bytes, and a backslash in front of any byte that is neither a letter nor a digit;
 *   \t \n \r \f \v \0 \xHH;   .   \d \w \s \D \W \S (ASCII);
 *   classes [...] with ranges, a leading ^, the escapes and shorthands above inside;
 *   groups ( ) and (?: ), both only grouping;   |   and the quantifiers * + ? {m} {m,} {m,n} on an atom or a group.
 * FHS_REGEX_IGNORE_CASE closes every positive set under the case swap of ASCII letters; a negated class is the
 * complement of the closed set.  Everything else is FHS_ERR_ARG before anything is recorded: anchors and \b \B \A \Z,
 * back-references and every other letter or digit escape, look-around, inline flags and named groups, lazy,
 * possessive and stacked quantifiers, a quantifier with nothing to repeat, a '{' that is not one of the three counted
 * forms, a NUL byte in pat, unbalanced brackets, an empty class ("[]", "[^]"), an unescaped '[' at the start of a class or a doubled
 * - & ~ | inside one, a range from or to a shorthand, a reversed range or {m,n}, unknown flag bits, a null out.
 * Counted repeats are expanded ({m,n}: n copies, {m,}: max(m, 1) copies; FHS_REGEX_SEARCH adds two positions): more than
 * FHS_REGEX_MAX_POSITIONS pattern positions, more than 1024 written atoms, groups and '|' together, or groups nested deeper than 64, are
 * FHS_ERR_LIMIT, and nothing is recorded; so is a full registry of user tables in fused mode, whose class and
 * step tables are registered before the string is loaded (as written none is registered).  A pattern whose shortest match is longer than n gives a trivial 0; one that
 * matches every text ('.*', a nullable pattern under FHS_REGEX_SEARCH), and a nullable pattern on n == 0, a trivial 1:
 * all with nothing recorded and no operand loaded.  Both modes; the fused DAG is as deep as the string is long (one level per character).
 * fhs_regex_info is the parser alone (no context): the number of positions and the length of the shortest match; for a
 * refused pattern *err_offset is the byte offset of the first byte of what is refused (the bracket that is never closed,
 * the second quantifier, the backslash of an escape; 0 for a limit).  Any of the three pointers may be null. */
#define FHS_REGEX_IGNORE_CASE 1
#define FHS_REGEX_SEARCH 2
#define FHS_REGEX_MAX_POSITIONS 64
int fhs_str_regex_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags, fhs_char_t *out);
int fhs_regex_info(const char *pat, size_t m, uint32_t flags, size_t *positions, size_t *min_len, size_t *err_offset);

/* ---- regular expressions: where the match is -------------------------------------------
 * With text = the n characters of s up to the first NUL (all of them if there is none), L = len(text) and
 *   rx = re.compile(pat, re.S)                       Python, bytes; re.I as well with FHS_REGEX_IGNORE_CASE
 * regex_starts_clear: out[i] is the 0/1 flag char of "i <= L and rx.match(text, i) is not None" -- a match begins at i,
 * and i lies inside the text; i == L can hold a 1 only for a nullable pattern (the empty match at the end) and L < n.
 * regex_find_clear: rx.search(text).start() as find_class returns a position -- the index of the first set start flag,
 * FHS_MAX_FIND_LENGTH (FHS_WIDE_ABSENT for the wide form) if there is no match; an index equal to that value reads the
 * same.  A match that exists only beyond the first NUL is not found.  No atom matches NUL, so a match that starts inside
 * the text ends inside it: any end will do, as under FHS_REGEX_SEARCH.  The syntax, its refusals and its limits are
 * fhs_str_regex_clear's; FHS_REGEX_IGNORE_CASE is the only flag bit -- the calls are searches by nature, so
 * FHS_REGEX_SEARCH is FHS_ERR_ARG like every unknown bit.  FHS_ERR_LIMIT above 256 (65536) characters for a position,
 * as for find_class.  A nullable pattern gives the trivial position 0; a pattern that is not nullable and whose shortest
 * match is longer than n (or n == 0) the trivial absent value and n trivial zero flags: all with nothing recorded and no
 * operand loaded.  Every error is raised before anything is recorded; fused mode registers its class and step tables
 * before the string is loaded (FHS_ERR_LIMIT when the registry is full), as written none is registered.  Both modes;
 * the automaton runs backwards over the string once, so the fused DAG is as deep as the string is long, plus the levels
 * of find_class's position for the two find forms. */
int fhs_str_regex_find_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags, fhs_char_t *out);
int fhs_str_regex_find_clear_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags, fhs_char_t *lo, fhs_char_t *hi);
int fhs_str_regex_starts_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags, fhs_char_t *out /*[n]*/);

/* ---- user look-up tables; clear tables and sets on strings -----------------------------
 * fhs_user_lut registers a 16-entry table f(v), v in [0, 16), values block values below 32, and returns its id in
 * *lut_id.  The registry is process-wide and interned by content: equal tables get the same id, ids count up from the
 * end of the built-in catalogue in order of first registration, and every context (planner contexts included) folds,
 * records and bootstraps with them like with a catalogue table.  A context expands the tables it uses on its GPU, next to
 * the catalogue, in front of the first launch group that names them; only the 16 bytes cross the bus.  Capacity:
 * 65536 minus the catalogue's size (table ids are 16 bits wide); past it FHS_ERR_LIMIT, and nothing is recorded.
 * FHS_ERR_ARG: a null pointer or a value above 31.  fhs_user_lut_count: tables registered so far;
 * fhs_lut_catalogue_count: the size of the built-in catalogue, the first user id. */
int fhs_user_lut(const uint8_t *values /*[16]*/, int *lut_id);
int fhs_user_lut_count(void);
int fhs_lut_catalogue_count(void);
/* diagnostic: the device copy of the polynomial [2048] of a catalogue or user table, what fhs_debug_lut_poly computes on
 * the host; a user table this context has not used yet is expanded first.  FHS_ERR_STATE on a planner context or
 * without a server key, FHS_ERR_ARG for an unknown id. */
int fhs_debug_read_lut(fhs_ctx *ctx, int lut_id, uint64_t *out /*[2048]*/);
/* A clear table or set applied to each of the n buffer characters as it is, NULs included; both modes.
 * map_clear: out[i] = table[s[i]], table[256].  class_flags: out[i] = the 0/1 flag char of "s[i] is in the set", set32 a
 * bitmap of 256 bits (byte x >> 3, bit x & 7).  find_class: the index of the first character in the set, as find
 * returns it (FHS_MAX_FIND_LENGTH / FHS_WIDE_ABSENT if there is none; an index equal to that value reads the same);
 * FHS_ERR_LIMIT above 256 (65536) characters, before anything is recorded.  Fused mode factors the table into user
 * tables: nothing for a digit that does not change, at most three bootstraps per digit in two levels where its 16 x 16
 * matrix over the nibbles has few distinct rows or columns, at most 192 per character otherwise; FHS_ERR_LIMIT when the
 * registry is full, before anything is recorded. */
int fhs_str_map_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *table /*[256]*/, fhs_char_t *out /*[n]*/);
int fhs_str_class_flags(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *set32 /*[32]*/, fhs_char_t *out /*[n]*/);
int fhs_str_find_class(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *set32 /*[32]*/, fhs_char_t *out);
int fhs_str_find_class_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *set32 /*[32]*/, fhs_char_t *lo, fhs_char_t *hi);

/* ---- multi-GPU inside the library (one process per GPU, RCCL over xGMI) ---------------------------------
 * north_star: "characters of an FheString are independent PBS batches, so long strings shard across the GPUs of one
 * node with an RCCL gather".  fhs_dist_init creates this context's communicator (librccl.so.1 is loaded at run time;
 * rank 0 obtains the 128-byte id with fhs_dist_unique_id and hands it to the other ranks by any means).  All
 * collectives are ncclAllGather calls enqueued on the context's own HIP stream: nothing waits on the host. */
#define FHS_DIST_ID_BYTES 128
int fhs_dist_unique_id(void *id /*[128]*/);
int fhs_dist_init(fhs_ctx *ctx, int rank, int world, const void *nccl_unique_id /*[128]*/);
/* Transport for ranks that SHARE one GPU (RCCL refuses two ranks on one device; tests on a one-GPU box): the library
 * stages through pinned host memory and calls `fn(user, send, recv, bytes_per_rank)` (0 = ok), e.g. a gloo all-gather. */
typedef int (*fhs_allgather_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank);
int fhs_dist_init_host_transport(fhs_ctx *ctx, int rank, int world, fhs_allgather_fn fn, void *user);
int fhs_dist_shutdown(fhs_ctx *ctx);
/* Teardown after a bring-up that did not succeed on EVERY rank (fhs_dist_init returned 0 here and an error elsewhere):
 * the half-formed communicator is aborted (ncclCommAbort: no exchange with the peers) instead of destroyed, nothing is
 * flushed or waited for.  fhs_dist_shutdown on such a communicator may block. */
int fhs_dist_abort(fhs_ctx *ctx);
/* 1 if librccl.so.1 can be loaded with every entry point used here (dlopen + dlsym only: no communicator is made, no
 * GPU is touched).  ncclCommInitRank is collective: agree on this among ALL ranks before any of them calls
 * fhs_dist_init, or the ranks that could load it block forever waiting for the one that could not. */
int fhs_dist_available(void);
/* Exchange counters of this context since fhs_dist_init*: all-gathers issued (ncclAllGather calls, or host-transport
 * callbacks), bytes THIS rank contributed, and which transport carries them. */
#define FHS_TRANSPORT_NONE 0
#define FHS_TRANSPORT_RCCL 1
#define FHS_TRANSPORT_HOST 2
int fhs_dist_stats(const fhs_ctx *ctx, uint64_t *n_allgather, uint64_t *bytes_sent, int *transport);
int fhs_dist_rank(const fhs_ctx *ctx);
int fhs_dist_world(const fhs_ctx *ctx);
/* Partition helpers (pure host logic).  Windows 0..n_chars-m of contains/find split into `world` contiguous ranges:
 * rank evaluates windows [*w0, *w1) and holds characters [*c0, *c1) (its slice plus an (m-1)-character halo).
 * Positions 0..n_chars split into `world` contiguous ranges [*c0, *c1) (eq / eq_ignore_case / comparisons). */
void fhs_dist_plan_windows(size_t n_chars, size_t m, int world, int rank, size_t *w0, size_t *w1, size_t *c0, size_t *c1);
void fhs_dist_plan_positions(size_t n_chars, int world, int rank, size_t *c0, size_t *c1);
/* Generic exchange: n chars (resp. n single-block flags) of every rank -> out[r * n + i] on every rank. */
int fhs_dist_allgather_chars(fhs_ctx *ctx, const fhs_char_t *local, size_t n, fhs_char_t *out /*[world * n]*/);
int fhs_dist_allgather_flags(fhs_ctx *ctx, const fhs_char_t *local, size_t n, fhs_char_t *out /*[world * n]*/);
/* Sharded string methods: `shard` is THIS rank's slice (fhs_dist_plan_*), patterns are replicated; every rank returns
 * the full result.  contains: mod.rs:151-182 (1 block exchanged per rank).  find: mod.rs:1010-1053, every rank
 * bootstraps the match flags of its windows (the two wide levels), ONE all-gather of ceil(W / world) blocks per rank hands
 * every rank all W flags, the narrow rest (prefix OR, index of the first flag) runs replicated: six dependency levels
 * like the single-GPU find; `shard` / `first_window` must be this rank's slice of fhs_dist_plan_windows(total_chars, m);
 * FHS_ERR_LIMIT when total_chars >= 255 + m like the reference's panic.  eq / eq_ignore_case:
 * mod.rs:1122-1149, :1221-1231 on equally long padded buffers (1 block).  compare: mod.rs:1470-1541, cmp 0 lt, 1 le,
 * 2 gt, 3 ge (2 blocks). */
int fhs_dist_str_contains(fhs_ctx *c, const fhs_char_t *shard, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out);
int fhs_dist_str_contains_clear(fhs_ctx *c, const fhs_char_t *shard, size_t n, const char *pat, size_t m, fhs_char_t *out);
int fhs_dist_str_find(fhs_ctx *c, const fhs_char_t *shard, size_t n, const fhs_char_t *pat, size_t m, size_t first_window,
                      size_t total_chars, fhs_char_t *out);
int fhs_dist_str_find_clear(fhs_ctx *c, const fhs_char_t *shard, size_t n, const char *pat, size_t m, size_t first_window,
                            size_t total_chars, fhs_char_t *out);
int fhs_dist_str_eq(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, int ignore_case,
                    fhs_char_t *out);
int fhs_dist_str_compare(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, int cmp, fhs_char_t *out);
/* Level-parallel mode for ANY op (replace with its compaction, ...): every rank holds the same ciphertexts and records
 * the same DAG; while on, fhs_flush / fhs_flush_async run slice [rank*cap, (rank+1)*cap) of every dependency level,
 * all-gather the level (cap x 16 392 B per rank) on the stream and install it -- all levels enqueued back to back. */
int fhs_dist_level_parallel(fhs_ctx *ctx, int on);

/* ---- level-parallel execution with a caller-provided collective (low-level protocol; SURVEY 5 "per-level") ----
 * Every rank holds the same ciphertexts and records the same DAG.  fhs_flush_plan levelises it;
 * for each level k every rank runs its slice [rank*cap, (rank+1)*cap) of the level's PBS
 * (cap = ceil(width / world)) into rows of `d_slice` (device, cap x 2049 u64), the caller all-gathers
 * the slices (RCCL) into `d_all` (world x cap x 2049) and fhs_flush_level_commit installs the results.
 * fhs_flush() refuses to run while world > 1 has pending work. */
int fhs_dist_config(fhs_ctx *ctx, int rank, int world);
int fhs_flush_plan(fhs_ctx *ctx, uint64_t *n_levels, uint64_t *max_level_width);
int fhs_flush_level_exec(fhs_ctx *ctx, uint64_t level, uint64_t *d_slice, uint64_t *width, uint64_t *cap);
int fhs_flush_level_commit(fhs_ctx *ctx, uint64_t level, const uint64_t *d_all);
int fhs_stream_sync(fhs_ctx *ctx);

/* ---- debug: capture of PBS inputs (noise-margin measurement; tests/test_gpu_noise.py) -------------
 * While enabled, every executed level copies a strided sample (at most max_rows_per_level rows) of its PBS inputs --
 * the linear-combination results that enter keyswitch -- to host memory, with the record below.  The caller
 * decrypts their phase with the client key; the library never sees a secret.  0 disables and clears. */
typedef struct {
    uint32_t level, index;     /* dependency level within its flush, position within the level */
    uint32_t lut;              /* LUT catalogue id of the PBS (csrc/luts.h) */
    uint32_t n_terms;          /* ciphertext terms of the linear combination */
    int64_t sum_c2;            /* sum of squared coefficients (noise amplification of the construct) */
    int32_t konst;             /* trivial constant added (mod 32) */
    uint32_t width;            /* PBS in this level */
} fhs_capture_rec;
int fhs_debug_capture_pbs_inputs(fhs_ctx *ctx, size_t max_rows_per_level);
/* on != 0: sample inside the ordinary execution path -- rotation sharing, round alignment and tick scheduling exactly as
 * in production (tests/test_gpu_margins.py); 0 (default): through an all-at-once plan without rotation sharing.  `level`
 * of a record then counts the job levels executed since the last fhs_reset_stats. */
int fhs_debug_capture_live(fhs_ctx *ctx, int on);
/* Copies up to `cap` captured rows ([2049] u64 each) and records, returns the number in *n and clears the capture;
 * rows == NULL only reports the count (nothing is cleared). */
int fhs_debug_capture_read(fhs_ctx *ctx, uint64_t *rows, fhs_capture_rec *recs, size_t cap, size_t *n);

/* ---- debug: plan trace of a planner context (tests/test_plan_exec.py; bench.py's CPU-baseline leg) --------------
 * While on, a planner context (fhs_ctx_create_planner: no device) writes what it WOULD run as 64-bit words; block tokens
 * are the planner's unique fake pointers:
 *   1 token                                    an uploaded block, in upload order
 *   2 out lut konst n (token coef) x n         one bootstrap: LUT `lut` of sum coef * block + konst * 2^59 -> block `out`
 *   3 leader_out out K                         a shared extraction: coefficient K of the accumulator of `leader_out`'s row
 *                                              (= that row's bootstrap with konst + K / 128)
 *   4 width                                    end of a launch group (its rows are independent of one another)
 * A host executor replays the list with any bootstrap implementation: the CPU oracle runs the product's fused DAGs on
 * real ciphertexts this way (oracle/plan_exec.py).  fhs_debug_char_terms describes a result handle after the flush, per
 * block: kind (0 plaintext, 1 block, 2 linear combination), value or konst, n, (token coef) x n.  fhs_debug_lut_poly:
 * the body polynomial [2048] of a LUT id (csrc/luts.h), of the catalogue or a registered user table (fhs_user_lut). */
int fhs_debug_plan_trace(fhs_ctx *ctx, int on);
int fhs_debug_plan_read(fhs_ctx *ctx, uint64_t *out, size_t cap, size_t *n);
int fhs_debug_char_terms(fhs_ctx *ctx, fhs_char_t h, uint64_t *out, size_t cap, size_t *n);
int fhs_debug_lut_poly(int lut_id, uint64_t *out);
/* Process-wide figures of what THIS library holds through its resource owners (nothing of another library or process:
 * the device-wide hipMemGetInfo cannot carry an exact assertion on a shared machine): out[0] live device bytes,
 * out[1] live pinned host bytes, out[2] live events, out[3] live streams, out[4] acquisitions since process start.
 * After every context is destroyed words 0..3 are zero; a planner context acquires nothing. */
int fhs_debug_live_resources(uint64_t out[5]);

/* ---- statistics ----------------------------------------------------------------
 * fhs_stats grows at its END when a counter is added (round 5: pbs_extracted): a host must be compiled against the
 * header of the library it loads -- fhs_get_stats writes sizeof(fhs_stats) bytes of THAT build.  (build() recompiles
 * examples/c_host for this reason; the generated Rust binding carries the same layout.) */
typedef struct {
    uint64_t pbs_executed;     /* PBS actually run on the GPU (constant-folded ones excluded) */
    uint64_t pbs_folded;       /* PBS on all-trivial inputs folded at DAG construction */
    uint64_t levels;           /* dependency levels launched */
    uint64_t max_level_width;
    uint64_t blocks_live;      /* device ciphertext blocks currently allocated */
    uint64_t max_input_sum_c2; /* largest sum of squared coefficients of a bootstrap's input (flattened linear
                                * combination of bootstrap outputs / uploads): its noise variance in units of one
                                * bootstrap output's.  The string layer keeps it <= FHS_NOISE_BUDGET_SUM_C2. */
    uint64_t pbs_shared;       /* fused mode: PBS not run because an identical one (same LUT on the same linear combination
                                * of the same blocks) already exists -- e.g. the high-nibble tests of one character
                                * against pattern characters that share their high nibble */
    uint64_t pbs_extracted;    /* results obtained as a further sample extraction of ANOTHER row's blind rotation (rotation
                                * sharing: same table, same combination up to its trivial constant); not in pbs_executed */
} fhs_stats;
/* Design rule of the fused DAGs: with a measured bootstrap-output sigma of 2^48.9 a sum with
 * sum c^2 <= 64 adds sigma <= 2^51.9 to the 2^55.2 of keyswitch + modulus switch (+0.8 %): the reference parameter
 * set's 2^-40 failure probability is kept (tests/test_gpu_noise.py measures it). */
#define FHS_NOISE_BUDGET_SUM_C2 64
int fhs_get_stats(fhs_ctx *ctx, fhs_stats *out);
/* Noise of a handle in the same unit: the largest sum of squared coefficients over its four blocks (0 trivial, 1 a
 * bootstrap output or an upload).  Results are handed back at <= 4 except the index of find / find_clear, whose digits
 * are sums of up to 57 bootstrap outputs (inside the decryption margin; saves one dependency level).  The library
 * refreshes a block above 4 by itself when its handle is used as an operand, also after a download (a linear
 * combination materialised for fhs_download / fhs_export_device keeps its figure).  A ciphertext that LEAVES the library
 * has to carry the figure with it, like the noise_level of a tfhe-rs shortint ciphertext travels in its serialised form
 * (tfhe 0.5.2, Cargo.lock:416-433): query it here before the download ... */
int fhs_char_sum_c2(fhs_ctx *ctx, fhs_char_t h, uint64_t *out);
/* ... and declare it after fhs_upload / fhs_upload_string of such a ciphertext (uploads count as 1 otherwise, the
 * figure of a fresh client encryption -- fheasciichar.rs:27-29).  Handles of uploaded (or trivial) blocks only; the
 * figure can be raised, never lowered below what the library tracks. */
int fhs_char_set_noise(fhs_ctx *ctx, fhs_char_t h, uint64_t sum_c2);
/* Constant folding made visible: *is_trivial = 1 and *value = the byte if all four blocks of the handle are trivial
 * (plaintext) ciphertexts -- what an operation on trivially encrypted inputs folds to, without a GPU (planner contexts
 * included).  The CPU tests evaluate the re-associated DAGs on every byte pair this way. */
int fhs_trivial_value(fhs_ctx *ctx, fhs_char_t h, int *is_trivial, uint8_t *value);
/* Width (PBS count) of every dependency level executed since the last fhs_reset_stats, in execution order (the shape
 * of the levelized batches: what a CPU baseline has to run to do the same work).  *n = number of levels; out may be
 * NULL to query it. */
int fhs_level_widths(fhs_ctx *ctx, uint32_t *out, size_t cap, size_t *n);
/* Rows THIS rank ran in every launch group (one lincomb -> keyswitch -> blind-rotation sequence) since the last
 * fhs_reset_stats, in order: several dependency levels may share a group (level-skewed batching, round alignment) and a
 * level-parallel rank runs its slice of each.  With a planner context that has a host transport attached
 * (fhs_dist_init_host_transport with any callback: it is never called) the sharded entry points can be RECORDED for any
 * (rank, world): groups, PBS, all-gathers and bytes of fhs_dist_stats are what a real run of that rank would issue --
 * the basis of tools/project_multi_gpu.py. */
int fhs_launch_groups(fhs_ctx *ctx, uint32_t *out, size_t cap, size_t *n);
int fhs_reset_stats(fhs_ctx *ctx);

/* ---- client side (MyClientKey, src/client_key.rs) -- host CPU, like the reference -- */
/* Keys, masks and noise come from ChaCha20 keyed with 256 bits of getrandom(2) entropy (the reference: tfhe-rs's
 * OS-seeded concrete-csprng); separate streams for secret keys, public masks and noise. */
int fhs_client_create(fhs_client **out);                                 /* from_params :30-35 */
/* TEST / BENCHMARK ONLY: the same generator keyed from a 64-bit seed -> reproducible keys and ciphertexts (identical
 * keys on every rank of a multi-GPU run, fixed test vectors).  At most 64 bits of entropy: never for real data. */
int fhs_client_create_insecure_seeded(uint64_t seed, fhs_client **out);
/* Diagnostic: one block of the generator's ChaCha20 (RFC 8439 2.3.2 known-answer test in tests/test_cabi.py). */
void fhs_chacha20_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]);
/* Diagnostic: n 64-bit draws from that state, i.e. the keystream of consecutive blocks in order (the generator makes
 * eight blocks at a time with AVX2 where the CPU has it: same stream as the scalar block function). */
void fhs_chacha20_stream(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint64_t *out, size_t n);
void fhs_client_destroy(fhs_client *ck);
const uint64_t *fhs_client_bsk(const fhs_client *ck);                    /* get_server_key :37-39 */
const uint64_t *fhs_client_ksk(const fhs_client *ck);
/* pair key of FHS_ARITH_F64_FFT_MB2 (generated on first call; FHS_BSK_MB2_WORDS words): for each pair of LWE key bits
 * (s, s') GGSW encryptions of s(1-s'), (1-s)s' and s s' */
const uint64_t *fhs_client_bsk_mb2(fhs_client *ck);
int fhs_client_encrypt_char(fhs_client *ck, uint8_t v, uint64_t *blocks /*[4][2049]*/); /* encrypt_char :85-87 */
int fhs_client_decrypt_char(const fhs_client *ck, const uint64_t *blocks, uint8_t *out); /* decrypt_char :81-83 */
/* encrypt :45-65 (ASCII, no NUL, `padding` NULs appended): out[(len+padding)][4][2049] */
int fhs_client_encrypt_str(fhs_client *ck, const char *s, size_t len, size_t padding, uint64_t *out);
/* decrypt :89-106 (truncates at the first NUL); returns the number of bytes written */
int fhs_client_decrypt_str(const fhs_client *ck, const uint64_t *chars, size_t n, char *out, size_t *out_len);
int fhs_client_secret_keys(const fhs_client *ck, uint64_t *lwe_sk /*[742]*/, uint64_t *glwe_sk /*[2048]*/);

/* ---- key files (the reference derives serde traits at client_key.rs:9 and
 * server_key/mod.rs:13 but never calls them).  Little-endian: 64-byte header {magic "FHSKEY01", kind,
 * lwe_n, poly_n, ks_levels, ks_base_log, pbs_base_log, bsk_quant_bits}, then raw u64 arrays.
 * kind 1 = client key (secret keys + server key), kind 2 = server key only (bsk, ksk), kind 4 = compressed server key,
 * kind 5 = packing key, kind 6 = public key, kind 7 = re-key key of the string store (all four below). */
int fhs_client_save(const fhs_client *ck, const char *path, int server_key_only);
int fhs_client_load(const char *path, fhs_client **out);             /* kind 1 files only */
int fhs_load_server_key_file(fhs_ctx *ctx, const char *path);        /* kind 1 or 2 */
/* kind 3 = the pair key of FHS_ARITH_F64_FFT_MB2 / FHS_ARITH_EXACT_NTT_MB2 alone (generated on first use): it travels
 * beside a kind 1 / 2 file and is loaded after it, converted for the arithmetic selected at that moment */
int fhs_client_save_multibit_key(fhs_client *ck, const char *path);
int fhs_load_multibit_key_file(fhs_ctx *ctx, const char *path);

/* ---- compressed (seeded) ciphertexts and server keys --------------------------------------------------------
 * The uniform mask of an LWE / GGSW row is drawn from a PUBLIC 256-bit seed, so only the body travels; the server
 * regenerates the mask (on the GPU: fhs_upload_string_compressed, fhs_load_compressed_server_key).  The seeded-stream
 * convention: every seeded row has its own ChaCha20 stream (RFC 8439 block function, the client generator's layout)
 *   key = the seed as uint32_t[8];  st[12] = block counter, from 0;  st[13] = domain;  st[14] / st[15] = stream id
 *   low / high;  draw k = keystream words (2k, 2k + 1), low word first (fhs_chacha20_stream's k-th value)
 * and
 *   string, character i (global index), block b   domain 4, stream 4i + b   draws 0..2047 = mask words 0..2047,
 *                                                                            the body (word 2048) is sent
 *   BSK, key bit i, GGSW row r                     domain 5, stream 2i + r   draws 0..2047, each & ~63 (the 58-bit
 *                                                                            grid) = the row's mask polynomial; the
 *                                                                            row's body polynomial is sent
 *   KSK, row i, level l                            domain 6, stream 5i + l   draws 0..741 = ct[0..741], ct[742] sent
 * Expanded layouts are exactly those of fhs_upload_string's input and of fhs_client_bsk / fhs_client_ksk.  Noise is
 * the classic encryption's (secret streams of the client, never reused), so a compressed upload counts as one fresh
 * encryption in the noise bookkeeping.  A seed reveals no secret generator state: it is OS entropy (an insecure seeded
 * client derives it from its 64-bit seed and the call number, never from its secret generator key).
 * Sizes: a character is 4 bodies (32 B) instead of 65 568 B, a string adds its 32-byte seed; the server key (kind 4
 * file) is 24 395 872 B instead of 109 MB.  Results: see "packed result download" below. */
#define FHS_DOM_SEEDED_STR 4
#define FHS_DOM_SEEDED_BSK 5
#define FHS_DOM_SEEDED_KSK 6
#define FHS_SEED_WORDS 8                                   /* uint32_t words of a seed */
#define FHS_CSTR_BODY_WORDS 4                              /* u64 words per character of a compressed string */
#define FHS_CBSK_BODY_WORDS ((size_t)742 * 2 * 2048)       /* [742][2 rows][2048] */
#define FHS_CKSK_BODY_WORDS ((size_t)2048 * 5)             /* [2048][5] */
#define FHS_CKEY_FILE_BYTES ((size_t)64 + 32 + 742 * 2 * 2048 * 8 + 2048 * 5 * 8)   /* kind 4 key file */
/* fhs_client_encrypt_str, compressed: same validation and limits; a fresh seed per call (seed_out) and
 * bodies[(len+padding)][4].  The mask is streamed into the dot product and never stored. */
int fhs_client_encrypt_str_compressed(fhs_client *ck, const char *s, size_t len, size_t padding, uint32_t seed_out[8],
                                      uint64_t *bodies);
/* Host reference expansion (public data only): characters first_char .. first_char + n - 1 of a compressed string,
 * bodies[n][4] = THOSE characters' bodies -> out[n][4][2049].  first_char: a rank's window of a sharded string
 * (fhs_dist_plan_windows). */
int fhs_expand_compressed_str(const uint32_t seed[8], const uint64_t *bodies, size_t n, size_t first_char, uint64_t *out);
/* Device expansion straight into the context's ciphertext blocks (16 B per block cross the bus: body and destination):
 * the seeded twin of fhs_upload_string, same arguments as fhs_expand_compressed_str.  A planner context records the
 * uploads and computes nothing. */
int fhs_upload_string_compressed(fhs_ctx *ctx, const uint32_t seed[8], const uint64_t *bodies, size_t n, size_t first_char,
                                 fhs_char_t *out);
/* A second valid server key of the client, compressed (generated on first call and kept, like the pair key): its masks
 * come from a public seed, its noise from secret streams of its own.  fhs_client_bsk / fhs_client_ksk do not change. */
int fhs_client_compressed_server_key(fhs_client *ck, uint32_t seed_out[8], uint64_t *bsk_bodies /*[742][2][2048]*/,
                                     uint64_t *ksk_bodies /*[2048][5]*/);
/* kind 4 key file: header, seed (32 B), BSK bodies, KSK bodies.  fhs_client_load, fhs_load_server_key_file and
 * fhs_load_multibit_key_file refuse it. */
int fhs_client_save_compressed_server_key(fhs_client *ck, const char *path);
/* Host reference expansion of a compressed server key to the standard-domain bsk[742][2][2][2048], ksk[2048][5][743]. */
int fhs_expand_compressed_server_key(const uint32_t seed[8], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies,
                                     uint64_t *bsk, uint64_t *ksk);
/* Expands on the device into what fhs_load_server_key fills (same pair-key invalidation, same arithmetic rules). */
int fhs_load_compressed_server_key(fhs_ctx *ctx, const uint32_t seed[8], const uint64_t *bsk_bodies,
                                   const uint64_t *ksk_bodies);
int fhs_load_compressed_server_key_file(fhs_ctx *ctx, const char *path);   /* kind 4 only */
/* Diagnostic: n draws of the DEVICE ChaCha20 from (key, counter, nonce) -- the same values as fhs_chacha20_stream,
 * including the counter's carry into nonce[0] (+0x100 per wrap). */
int fhs_debug_chacha20_device(fhs_ctx *ctx, const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint64_t *out,
                              size_t n);

/* ---- packed result download ---------------------------------------------------------------------------------
 * Up to 2048 result blocks (512 characters) leave the server as ONE GLWE ciphertext under the client's GLWE key
 * (N = 2048, k = 1), block j of the group in coefficient j, stored at 16 bits per word: a group is a 2048 x u16 mask and
 * one u16 body per block present -- 4096 * ceil(4n / 2048) + 8n bytes for n characters (4097 characters: 69 640 B
 * instead of 268 632 096 B).  The big LWE key of a block IS the flattened GLWE key, so the packing is the ring packing
 * of Chen, Dai, Kim, Song (PackLWEs: 11 tree levels, one automorphism keyswitch per node) and the only new key material
 * is 11 automorphism keyswitch keys (FHS_PACK_KEY_WORDS words, ~1 MB):
 *   key[lv - 1][l] = (mask[2048], body[2048]): GLWE encryption of S(X^(2^lv + 1)) * 2^(64 - FHS_PACK_BASE_LOG (l + 1)),
 *   lv = 1..11, l < FHS_PACK_LEVELS, on the bootstrapping key's 58-bit grid, body = mask * S + message + noise.
 * All packing arithmetic is exact in Z_2^64[X]/(X^2048 + 1), whatever fhs_set_arithmetic selects: device and host
 * reference agree in every word.  mask16 / body16 arguments are arrays of uint16_t (host byte order), passed as void
 * pointers. */
#define FHS_PACK_BASE_LOG 16
#define FHS_PACK_LEVELS 3
#define FHS_PACK_TREE_LEVELS 11
#define FHS_PACK_GROUP 2048                                /* blocks per packed GLWE */
#define FHS_PACK_KEY_WORDS ((size_t)11 * 3 * 2 * 2048)     /* [11][FHS_PACK_LEVELS][mask, body][2048] */
#define FHS_PACK_KEY_FILE_BYTES ((size_t)64 + 11 * 3 * 2 * 2048 * 8)   /* kind 5 key file */
/* The packing key of the client (generated on first call and kept; fhs_client_bsk / fhs_client_ksk do not change). */
const uint64_t *fhs_client_packing_key(fhs_client *ck);
/* kind 5 key file: header + the packing key.  It travels beside a kind 1 / 2 / 4 file, like kind 3; every other loader
 * refuses it. */
int fhs_client_save_packing_key(fhs_client *ck, const char *path);
int fhs_load_packing_key(fhs_ctx *ctx, const uint64_t *key /*[FHS_PACK_KEY_WORDS]*/);
int fhs_load_packing_key_file(fhs_ctx *ctx, const char *path);   /* kind 5 only */
/* Sizes of the packed form of n_chars characters: u16 words of mask (2048 per group) and of body (4 per character). */
void fhs_packed_bytes(size_t n_chars, size_t *mask_words, size_t *body_words);
/* fhs_download_string, packed: mask16[ceil(4n / 2048)][2048], body16[4n] (group g's bodies start at 2048 g).  Takes any
 * handle fhs_download takes and leaves it unchanged.  FHS_ERR_STATE without a packing key or on a planner context. */
int fhs_download_string_packed(fhs_ctx *ctx, const fhs_char_t *chars, size_t n, void *mask16, void *body16);
/* Diagnostic: the same, plus the 64-bit packed GLWEs before the storage switch, mask64 / body64 [ceil(4n/2048)][2048]. */
int fhs_debug_download_string_packed64(fhs_ctx *ctx, const fhs_char_t *chars, size_t n, void *mask16, void *body16,
                                       uint64_t *mask64, uint64_t *body64);
/* Host reference (public data only, no GPU): blocks[n][2049] -> the 64-bit packed GLWEs mask64 / body64
 * [ceil(n / 2048)][2048]; absent blocks of the last group count as zero. */
int fhs_pack_host(const uint64_t *key, const uint64_t *blocks, size_t n_blocks, uint64_t *mask64, uint64_t *body64);
/* Storage switch of the host reference: every word -> ((x + 2^47) >> 48) & 0xffff; mask16[groups][2048], body16[n_blocks]. */
int fhs_pack_switch16(const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, void *mask16, void *body16);
/* Diagnostic: one tree node of the host reference, level lv = 1..11: out = P + AutoKS_g(M) with T = X^(2048 >> lv) * O,
 * P = E + T, M = E - T, g = 2^lv + 1; every argument a GLWE as mask[2048] | body[2048]. */
int fhs_debug_pack_node(const uint64_t *key, int lv, const uint64_t *e /*[2][2048]*/, const uint64_t *o, uint64_t *out);
/* Diagnostic: n single blocks with the given values mod 32 (message, carry and padding bits as they are) from the
 * client's sequential streams, like fhs_client_encrypt_char: blocks[n][2049]. */
int fhs_client_encrypt_blocks(fhs_client *ck, const uint8_t *values, size_t n, uint64_t *blocks);
/* Client side: semantics of fhs_client_decrypt_str (truncates at the first NUL) on the packed form of n_chars
 * characters ... */
int fhs_client_decrypt_packed_str(const fhs_client *ck, const void *mask16, const void *body16, size_t n_chars,
                                  char *out, size_t *out_len);
/* ... and every block's value mod 32 (message and carry bits, padding bit included), out[n_blocks]. */
int fhs_client_decrypt_packed_blocks(const fhs_client *ck, const void *mask16, const void *body16, size_t n_blocks,
                                     uint8_t *out);
/* The same two on a WINDOWED packed form ("packed download of parked entries" below): block i is coefficient
 * (first_coef + i) % 2048 of mask (first_coef + i) / 2048, mask16[ceil((first_coef + n_blocks) / 2048)][2048],
 * body16[n_blocks].  first_coef = 0 is the form above and the two functions above are that case.  FHS_ERR_ARG unless
 * first_coef is a multiple of 4 below 2048. */
int fhs_client_decrypt_packed_str_at(const fhs_client *ck, const void *mask16, const void *body16, uint32_t first_coef,
                                     size_t n_chars, char *out, size_t *out_len);
int fhs_client_decrypt_packed_blocks_at(const fhs_client *ck, const void *mask16, const void *body16, uint32_t first_coef,
                                        size_t n_blocks, uint8_t *out);

/* ---- public-key encryption: compact strings expanded on the GPU --------------------------------------------
 * Anyone who holds the client's PUBLIC key can encrypt a string this library computes on (the reference hands one out:
 * PublicKey::new / PublicParameters, client_key.rs:30-43).  The big LWE key of a block is the flattened GLWE key S, so
 * the public key is one RLWE sample in R = Z_2^64[X]/(X^2048 + 1),
 *   A = 2048 draws of the ChaCha20 stream of a PUBLIC 256-bit seed (the seeded-stream convention above), domain 7,
 *       stream 0;   B = A S + E   (E: the GLWE noise, from a secret stream of the client),
 * 32 B + 16 384 B in all, and one GLWE ciphertext under it carries 2048 blocks = 512 characters.  Block t = 4 x
 * character + digit of a string sits in group g = t / 2048 at coefficient j = t % 2048.  Per group the encryptor draws
 * U (uniform binary) and E1, E2 (GLWE noise) and sends
 *   mask = A U + E1,   body = B U + E2 + sum_j m_j 2^59 X^j      (wrapping 64-bit arithmetic)
 * with every word stored at 32 bits, (x + 2^31) >> 32: mask32[ceil(4n / 2048)][2048] and body32[4n] (group g's bodies
 * start at 2048 g), 8192 ceil(4n / 2048) + 16 n bytes for n characters (4097 characters: 139 280 B).  The server turns
 * block (g, j) into a classic 2049-word block by sample extraction, words widened by << 32:
 *   a_i = A_g[j - i] for i <= j,   a_i = -A_g[2048 + j - i] for i > j,   b = B_g[j]      (A_g, B_g: the group's mask, body)
 * Noise of an expanded block: E U - E1 S + E2 and the storage rounding, sigma ~ 2^35.2 against a bootstrap output's
 * 2^48.9, so a public-key upload counts as one fresh encryption (sum c^2 = 1) like every other upload (DESIGN.md
 * section 12).  Not wire compatible with tfhe-rs's CompactPublicKey / CompactCiphertextList, whose roles these play. */
#define FHS_DOM_PUBLIC_KEY 7
#define FHS_PK_BODY_WORDS 2048                             /* u64 words of B */
#define FHS_PK_GROUP 2048                                  /* blocks per public-key GLWE */
#define FHS_PK_FILE_BYTES ((size_t)64 + 32 + 2048 * 8)     /* kind 6 key file */
/* The client's public key (generated on first call and kept, like the packing key). */
int fhs_client_public_key(fhs_client *ck, uint32_t seed_out[8], uint64_t *body_out /*[2048]*/);
/* kind 6 key file: header, seed (32 B), B.  Every other loader refuses it. */
int fhs_client_save_public_key(fhs_client *ck, const char *path);
/* A public-key handle holds NO secret; it is an opaque pointer and nothing below takes an fhs_client.
 * fhs_public_key_load reads kind 6 files only. */
int fhs_public_key_create(const uint32_t seed[8], const uint64_t *body /*[2048]*/, void **pk_out);
int fhs_public_key_load(const char *path, void **pk_out);
void fhs_public_key_destroy(void *pk);
/* The handle's key back: seed_out[8], body_out[2048]. */
int fhs_public_key_get(const void *pk, uint32_t seed_out[8], uint64_t *body_out);
/* TEST ONLY: the encryptor's randomness (U, E1, E2) comes from this 64-bit seed and the number of calls since, instead
 * of a ChaCha key drawn from getrandom(2) per call. */
int fhs_public_key_set_insecure_seed(void *pk, uint64_t seed);
/* u32 words of mask (2048 per group) and of body (4 per character) of n_chars characters. */
void fhs_public_str_words(size_t n_chars, size_t *mask_words, size_t *body_words);
/* Host, no secret, no GPU.  The input rules of fhs_client_encrypt_str (ASCII, no NUL, `padding` NULs appended);
 * mask32 / body32 are arrays of uint32_t sized by fhs_public_str_words(len + padding). */
int fhs_public_encrypt_str(void *pk, const char *s, size_t len, size_t padding, void *mask32, void *body32);
/* Host reference expansion (public data only): characters first_char .. first_char + count - 1 of a string of n_total
 * characters, mask32 / body32 = the WHOLE string's -> out[count][4][2049]. */
int fhs_expand_public_str(const void *mask32, const void *body32, size_t n_total, size_t first_char, size_t count,
                          uint64_t *out);
/* Device expansion straight into the context's ciphertext blocks, same arguments: only the masks of the groups the
 * window touches, its bodies and the destinations cross the bus.  A planner context records the uploads and computes
 * nothing. */
int fhs_upload_string_public(fhs_ctx *ctx, const void *mask32, const void *body32, size_t n_total, size_t first_char,
                             size_t count, fhs_char_t *out);

/* ---- device-resident string store: strings parked packed, expanded on demand --------------------------------
 * A string a context keeps between requests costs 65 568 B of HBM per character as pool blocks.  The store parks it as
 * the output of the packing tree above with every word rounded to 32 bits, (x + 2^31) >> 32 -- word for word the compact
 * string format of the public-key uploads -- and the sample extraction of fhs_upload_string_public brings it back, whole
 * or by window, straight from device memory: 34 B per character at rest (4097 characters: 139 280 B instead of 268 MB).
 * An ENTRY is one block sequence: block t = 4 x character + digit sits in group t / 2048 at coefficient t % 2048, stored
 * as mask32[ceil(4n / 2048)][2048] followed by body32[4n] (the sizes of fhs_public_str_words) in ONE device allocation
 * of exactly that size.  Ids are non-zero and never reused inside a context.  A table of short strings is parked as ONE
 * entry (concatenated) and read by window; there is no per-string entry table.  Entries survive a server-key reload,
 * like handles, and die with the context.
 * Noise: a restored block carries the packing noise, sigma 2^43.1 (the 32-bit rounding's 2^35.2
 * disappears under it) against a bootstrap output's 2^48.9, i.e. 2^-11.6 of one sum c^2 unit per packing, which the
 * integer figure cannot show.  The store therefore keeps per block, on the host: the figure of fhs_char_sum_c2 at put (a
 * sum is materialised and keeps its figure; a TRIVIAL block is packed as the trivial leaf it is and comes back as an
 * ordinary ciphertext with figure 1: constant folding does not survive parking), the rotation group (members of one
 * shared blind rotation stay charged as fully correlated, also across windows read at different times), and the number
 * of packings inside the block's noise, `cycles`.  put stores the block's count + 1 and refuses a block that would
 * exceed FHS_STORE_MAX_CYCLES with FHS_ERR_LIMIT; get hands the count back to the block; a sum takes the maximum over
 * its terms; every bootstrap starts at 0 again.  The true variance of a block is <= figure x (1 + cycles x 2^-11.6), and
 * at 16 cycles sqrt(16) x 2^43.1 = 2^45.1 stays below the 2^46 that bounds packing noise: the limit only ever meets data
 * that is parked and re-parked without being computed on. */
#define FHS_STORE_MAX_CYCLES 16
/* Parks n characters (any handle fhs_download takes; they are left as fhs_download_string_packed leaves them, and the
 * caller releases them when it wants the pool blocks back).  *id_out receives the entry id.  FHS_ERR_STATE without a
 * packing key (also after a server-key reload dropped it), FHS_ERR_ARG for n = 0, FHS_ERR_LIMIT see above.  A planner
 * context records the bookkeeping and allocates nothing. */
int fhs_store_put(fhs_ctx *ctx, const fhs_char_t *chars, size_t n, uint64_t *id_out);
/* Characters [first_char, first_char + count) of an entry as FRESH handles (out[count]) owned by the caller: only the
 * destination pointers cross the bus (8 B per block).  Needs no key.  FHS_ERR_ARG for an unknown id or a window outside
 * the entry.  A planner context records one upload per block. */
int fhs_store_get(fhs_ctx *ctx, uint64_t id, size_t first_char, size_t count, fhs_char_t *out);
int fhs_store_drop(fhs_ctx *ctx, uint64_t id);                 /* frees the allocation; FHS_ERR_ARG for an unknown id */
/* Characters and bytes of device memory of one entry (8192 ceil(4n / 2048) + 16 n) / of all entries of the context. */
int fhs_store_info(fhs_ctx *ctx, uint64_t id, size_t *n_chars, size_t *device_bytes);
int fhs_store_stats(fhs_ctx *ctx, size_t *entries, size_t *chars, size_t *device_bytes);
/* An entry to host memory and back (disk, another context of the same client key).  mask32 / body32: arrays of uint32_t
 * sized by fhs_public_str_words(n).  meta[4n], one word per block: bits 0-15 the figure (>= 1), bits 16-23 cycles
 * (<= FHS_STORE_MAX_CYCLES), bits 24-31 zero, bits 32-63 the rotation group, renumbered 1..k within the entry (0 = none);
 * import draws k fresh groups.  import is one host-to-device copy and no kernel.  meta == NULL declares every block a
 * fresh upload (figure 1, no group, cycles 0): a public-key encrypted string can be parked as it arrives, without ever
 * being expanded whole.  import checks the ranges above and otherwise TRUSTS the figures, as fhs_char_set_noise trusts
 * its caller.  export: FHS_ERR_STATE on a planner context (it holds no ciphertext). */
int fhs_store_export(fhs_ctx *ctx, uint64_t id, void *mask32, void *body32, uint64_t *meta /*[4n]*/);
int fhs_store_import(fhs_ctx *ctx, const void *mask32, const void *body32, const uint64_t *meta /*may be NULL*/, size_t n,
                     uint64_t *id_out);
/* Host reference of the store's storage switch, next to fhs_pack_switch16: every word -> (x + 2^31) >> 32;
 * mask32[groups][2048], body32[n_blocks]. */
int fhs_pack_switch32(const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, void *mask32, void *body32);

/* ---- string store: re-keying parked entries to another client key -------------------------------------------
 * An entry is a plain GLWE ciphertext under its client's GLWE key S_old, 32 bits per word.  One GLWE keyswitch per group
 * of 2048 blocks -- the AutoKS of the packing tree without the automorphism -- moves it under the key S_new of another
 * client (a key rotation, or handing a parked string to a second client) without the secret-key holder touching the
 * data: exact arithmetic in R = Z_2^64[X]/(X^2048 + 1), a 64 KB key, no bootstrap, no pool blocks.
 * The RE-KEY KEY from S_old to S_new has FHS_REKEY_LEVELS digit levels of FHS_REKEY_BASE_LOG bits:
 *   key[l] = (mask[2048], body[2048]),  body = mask * S_new + noise + S_old * 2^(64 - FHS_REKEY_BASE_LOG (l + 1)),
 * on the bootstrapping key's 58-bit grid with the GLWE noise.  Per group (mask32[2048], body32[count]):
 *   A = mask32 << 32 = d_0 2^48 + d_1 2^32 with balanced digits in [-2^15, 2^15) (a stored mask word has exactly 32
 *   significant bits: no rounding; a carry out of d_0 is a multiple of 2^64),  Sum_col = sum_l d_l * key[l].col,
 *   mask' = -Sum_mask,  body'_j = (body32_j << 32) - Sum_body,j for j < count;  every word stored as (x + 2^31) >> 32.
 * The result is an entry in the same format under S_new: fhs_store_get / fhs_expand_public_str take it unchanged.
 * Noise: the keyswitch adds sigma 2^32.6 and the second 32-bit rounding 2^35.2, 2^-15 of the packing variance, so a
 * re-key changes neither the figure, nor the rotation group, nor `cycles` of a block; it is counted per entry, on the
 * host, and the re-key after the FHS_STORE_MAX_REKEYS-th of one entry is refused with FHS_ERR_LIMIT.  export / import do
 * not carry the counter (the meta word keeps its layout, bits 24-31 stay zero): an IMPORTED entry starts at 0 again.
 * A context CANNOT TELL which client key an entry is under: re-keying an entry with a key that starts from another
 * client's S, re-keying it twice, or mixing entries of two clients in one operation gives garbage without any error.
 * Keeping track is the caller's business.
 * Randomness of a re-key key: its masks and noise come from a ChaCha20 key drawn from getrandom(2) for that call alone
 * (streams l, domains 2 = masks / 3 = noise of that key), like the encryptor of fhs_public_encrypt_str: two keys into
 * the same `to`, from whatever `from`, never share a mask or noise (their difference would show (S_a - S_b) 2^k in the
 * clear).  When `to` is an insecure seeded client the ChaCha key is derived from `to`'s 64-bit seed, a tag of its own and
 * the number of re-key keys `to` has received so far (tests only). */
#define FHS_REKEY_BASE_LOG 16
#define FHS_REKEY_LEVELS 2
#define FHS_REKEY_KEY_WORDS ((size_t)2 * 2 * 2048)           /* [FHS_REKEY_LEVELS][mask, body][2048] */
#define FHS_REKEY_KEY_FILE_BYTES ((size_t)64 + 2 * 2 * 2048 * 8)   /* kind 7 key file */
#define FHS_STORE_MAX_REKEYS 255
/* The key that moves entries of `from` under the key of `to`.  Both secret keys are needed: the two clients are one
 * party, or `from` hands its client key to `to`.  A fresh key per call. */
int fhs_client_rekey_key(fhs_client *from, fhs_client *to, uint64_t *key_out /*[FHS_REKEY_KEY_WORDS]*/);
/* kind 7 key file: header + a fresh re-key key.  Every other loader refuses it. */
int fhs_client_save_rekey_key(fhs_client *from, fhs_client *to, const char *path);
/* The key is independent of the server key but needs its transform tables, so it is loaded after fhs_load_server_key and
 * dropped by a server-key reload exactly as the packing key is: one rule for auxiliary keys.  key == NULL unloads it.
 * A planner context records that a key is present and converts nothing. */
int fhs_load_rekey_key(fhs_ctx *ctx, const uint64_t *key /*[FHS_REKEY_KEY_WORDS], or NULL*/);
int fhs_load_rekey_key_file(fhs_ctx *ctx, const char *path);     /* kind 7 only */
/* Re-keys entry `id` with the loaded key: one kernel launch over all its groups on the context's stream, behind every
 * queued fhs_store_get.  id_out == NULL: in place -- id, size and allocation stay.  Otherwise a NEW entry in a new
 * allocation of its exact size receives the result (*id_out) and the original is untouched: the copy for a second
 * client.  It inherits figure / cycles / rotation groups verbatim and the original's re-key count + 1.
 * FHS_ERR_ARG: unknown id.  FHS_ERR_STATE: no re-key key on a device context.  FHS_ERR_LIMIT: see above.  A planner
 * context does the bookkeeping only and needs no key. */
int fhs_store_rekey(fhs_ctx *ctx, uint64_t id, uint64_t *id_out /*may be NULL*/);
int fhs_store_rekey_count(fhs_ctx *ctx, uint64_t id, uint32_t *n);
/* Host reference (public data only, no GPU): the same words as the device.  mask32 / body32 as in fhs_store_export
 * (uint32_t arrays sized for n_blocks blocks: ceil(n_blocks / 2048) x 2048 mask words, n_blocks bodies); the output
 * arrays may be the input arrays. */
int fhs_rekey_host(const uint64_t *key, const void *mask32, const void *body32, size_t n_blocks, void *mask32_out,
                   void *body32_out);
/* Diagnostic: the device kernel on raw words of ANY block count (an entry holds whole characters, 4 blocks each), same
 * arguments and aliasing rule as fhs_rekey_host.  FHS_ERR_STATE without a re-key key or on a planner context. */
int fhs_debug_rekey_device(fhs_ctx *ctx, const void *mask32, const void *body32, size_t n_blocks, void *mask32_out,
                           void *body32_out);

/* ---- packed result download under a recipient's key ----------------------------------------------------------
 * A result computed under client a's server key can leave the server under client b's key: the packing tree runs as for
 * fhs_download_string_packed (a's packing key), and the re-key key a -> b of the section above -- the same key, the same
 * format, kind 7 file -- switches its level-11 GLWE (M64[2048], B64[2048]) of every group of up to 2048 blocks to S_b in
 * place of the storage switch.  Exact, wrapping 64-bit words in R = Z_2^64[X]/(X^2048 + 1):
 *   a = (M64 + 2^31) >> 32 (fhs_pack_switch32's word; a carry out of the top wraps to 0),
 *   a << 32 = d_0 2^48 + d_1 2^32 with the balanced digits above,  Sum_col = sum_l d_l * key[l].col,
 *   mask16 = ((-Sum_mask + 2^47) >> 48) & 0xffff,   body16_j = ((B64_j - Sum_body,j + 2^47) >> 48) & 0xffff for j < count.
 * The body is not rounded on the way in: one rounding, fhs_pack_switch16's, at the end.  The output has the layout of
 * fhs_download_string_packed and b decrypts it with the unchanged fhs_client_decrypt_packed_str / _blocks.
 * Noise: packing 2^43.1, the mask's 32-bit rounding 2^35.2 and the keyswitch 2^32.6 all disappear under the final 16-bit
 * rounding, 2^48 sqrt((1 + |S_b|^2) / 12) ~ 2^51.2, the term that dominates an own-key download too: the decode margin
 * against 2^58 is the one of the packed download.  Handles and their figures are left as they are.
 * A context CANNOT TELL which client key its blocks are under, nor which key the loaded re-key key starts from or leads
 * to: a recipient download of blocks that are not under the `from` key of the loaded key (after a server-key switch, or
 * of a string restored from an entry that was re-keyed) gives garbage without any error.  Keeping track is the caller's
 * business. */
/* fhs_download_string_packed for the recipient of the loaded re-key key; takes what it takes and leaves the handles
 * unchanged.  mask64 / body64 (both or neither, may be NULL): the level-11 GLWEs under the SENDER's key, as
 * fhs_debug_download_string_packed64 gives them, so that a caller can check the device words against
 * fhs_rekey_packed_host.  n = 0 returns 0 in every state.  FHS_ERR_STATE: a planner context, no packing key, or no
 * re-key key (fhs_last_error says which). */
int fhs_download_string_packed_for(fhs_ctx *ctx, const fhs_char_t *chars, size_t n, void *mask16, void *body16,
                                   uint64_t *mask64 /*may be NULL*/, uint64_t *body64 /*may be NULL*/);
/* Host reference (public data only, no GPU): the same words as the device.  mask64 / body64 [ceil(n_blocks / 2048)][2048]
 * as fhs_pack_host produces them; mask16[ceil(n_blocks / 2048)][2048], body16[n_blocks] as fhs_pack_switch16 writes
 * them (bodies beyond n_blocks are not written). */
int fhs_rekey_packed_host(const uint64_t *key, const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, void *mask16,
                          void *body16);
/* Diagnostic: the device kernel alone on raw words of ANY block count, one launch over all groups, arguments of
 * fhs_rekey_packed_host.  FHS_ERR_STATE without a re-key key or on a planner context. */
int fhs_debug_rekey_packed_device(fhs_ctx *ctx, const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, void *mask16,
                                  void *body16);

/* ---- string store: packed download of parked entries, own or recipient key -----------------------------------
 * An entry already IS the output of the packing tree, one GLWE per 2048 blocks at 32 bits per word, so it leaves the
 * server without being expanded: its words are rounded to 16 bits -- through the re-key keyswitch on the way when a
 * recipient is to open it -- and 17 B per character cross the bus.  No pool block, no packing key,
 * no tree; the entry, its re-key counter and every figure stay as they are.
 * WINDOWED PACKED FORM of characters [first_char, first_char + count): the blocks are t0 = 4 first_char .. t0 + 4 count - 1;
 * with g0 = t0 / 2048 and g1 = (t0 + 4 count - 1) / 2048,
 *   mask16[g1 - g0 + 1][2048]: the masks of the covering groups;   body16[4 count]: the bodies of the window's blocks only;
 *   first_coef = t0 % 2048 (a multiple of 4): block i of the window is coefficient (first_coef + i) % 2048 of mask
 *   (first_coef + i) / 2048.
 * With first_char = 0 this is the layout of fhs_download_string_packed word for word.  A recipient who is handed a window
 * holds the masks of whole groups but the bodies of the window alone: the other rows of a table parked as one entry stay
 * closed to them.  Arithmetic, exact in wrapping 64-bit words, on w = the entry's 32-bit word:
 *   own key:    every word ((w + 2^15) >> 16) & 0xffff = fhs_pack_switch16 of w << 32 (a carry out of the top wraps to 0);
 *   recipient:  per covering group the keyswitch of fhs_store_rekey (the digits of mask32 are exact),
 *               mask16 = ((-Sum_mask + 2^47) >> 48) & 0xffff,  body16_j = (((body32_j << 32) - Sum_body,j + 2^47) >> 48) & 0xffff
 *               for the window's coefficients j of that group = fhs_rekey_packed_host of (mask32 << 32, body32 << 32).
 * Noise: the 16-bit rounding, sigma ~ 2^51.2, dominates as in every packed download; the entry's own 2^43.1 (after put)
 * or 2^35.2 (a public-key import) and the keyswitch's 2^32.6 disappear under it.  As everywhere, a context cannot tell
 * which key an entry is under: a recipient download of an entry that is not under the `from` key of the loaded re-key
 * key gives garbage without any error. */
/* u16 words of mask and body of the window and its first_coef (any of the three may be NULL); count = 0: no words. */
void fhs_store_packed_words(size_t first_char, size_t count, size_t *mask_words, size_t *body_words, uint32_t *first_coef);
/* One kernel launch on the context's stream, behind every queued fhs_store_get / fhs_store_rekey of the entry, two
 * device-to-host copies, one stream sync.  recipient != 0: under the key the loaded re-key key leads to.  FHS_ERR_ARG: unknown
 * id or a window outside the entry.  count = 0 returns 0 and writes nothing.  FHS_ERR_STATE: a planner context (it holds
 * no ciphertext), or recipient without a re-key key.  A packing key is NOT required. */
int fhs_store_download_packed(fhs_ctx *ctx, uint64_t id, size_t first_char, size_t count, int recipient, void *mask16,
                              void *body16);
/* Host reference (public data only, no GPU): the same words as the device.  mask32 / body32: the WHOLE entry as
 * fhs_store_export gives it, n_blocks_entry = 4 x its characters; rekey_key == NULL: the entry's own key.  mask16 / body16
 * sized by fhs_store_packed_words; no word outside them is written.  FHS_ERR_ARG for a window outside the entry. */
int fhs_store_packed_host(const uint64_t *rekey_key /*[FHS_REKEY_KEY_WORDS], or NULL*/, const void *mask32, const void *body32,
                          size_t n_blocks_entry, size_t first_char, size_t count, void *mask16, void *body16);

/* ---- string store: fetching a row by encrypted index --------------------------------------------------------
 * Every read above names its window in the clear: the server learns which row of a parked table a client fetches.  Here
 * the client sends the bits of its row index as GGSW ciphertexts under its own GLWE key and the server selects the row
 * with CMuxes on the entry's GLWEs: no bootstrap, no pool block, no server key, no auxiliary key.
 * GEOMETRY.  Entry `id` of n characters is read as R = n / row_chars rows; row_chars is a power of two in
 * 1..FHS_SELECT_MAX_ROW_CHARS, n a multiple of it and R >= 2, otherwise FHS_ERR_ARG (rows longer than a group are not
 * built).  A row is 4 row_chars consecutive blocks, so a group of 2048 blocks holds 2^r rows, r = log2(512 / row_chars).
 * The index p has bits = ceil(log2 R) bits, bit 0 least significant: with G = ceil(4n / 2048) > 1 groups the low r bits
 * rotate inside a group and the bits - r = ceil(log2 G) bits above them pick the group; with one group only the
 * ceil(log2 R) rotate bits exist.  fhs_store_select_bits returns `bits`, or 0 for a refused shape.
 * ORDER OF WORK (fixed).  1. The tree: level t = 0, 1, .. pairs nodes (2i, 2i + 1) of the level below (level 0: the
 * entry's groups) under bit r + t, node i of the next level = CMux(bit, node 2i, node 2i + 1); a missing right sibling is
 * the zero GLWE.  2. Then for k = 0 .. (rotate bits) - 1:  G <- CMux(bit k, G, X^(-4 row_chars 2^k) G), where
 * (X^-s G)_n = G_(n + s) for n + s < 2048 and -G_(n + s - 2048) otherwise.
 * ONE CMux of 32-bit GLWEs a, b (mask32[2048], body32[2048]; body words an entry does not store -- the tail of a partial
 * last group -- count as 0), exact in wrapping words in R = Z_2^64[X]/(X^2048 + 1):
 *   D = (b - a) mod 2^32 word by word, mask and body;  D << 32 = d_0 2^48 + d_1 2^32 with the balanced 16-bit digits of
 *   the re-key section (no rounding on the way in);  with the four digit polynomials l = 0..3 = mask d_0, mask d_1,
 *   body d_0, body d_1 and the four rows of the bit's GGSW,
 *   out_col = ((a_col << 32) + sum_l d_l * GGSW[l].col + 2^31) >> 32      for col = mask, body.
 * Every level stores 32-bit words, so every level is the same operation.
 * RESULT: a NEW entry of row_chars characters -- one group, mask32[2048] and body32[4 row_chars] = coefficients
 * 0 .. 4 row_chars - 1 of the last CMux; fhs_store_get / _rekey / _download_packed (own key or recipient) / _export take it
 * unchanged.  The source entry is only read.
 * AN INDEX p >= R is the caller's error and is not detected: the words are still deterministic and equal to the host
 * reference's; where whole tree nodes are missing the characters are NUL, inside a partial last group they are
 * unspecified.  As everywhere, a context CANNOT TELL which key an entry or a query is under: a query made by another
 * client, or for another shape, gives garbage without any error.
 * THE QUERY is `bits` GGSW ciphertexts, [bit][row: mask d_0, mask d_1, body d_0, body d_1][mask, body][2048] u64 words.
 * A row is (mask, body = mask * S + e + m) on the bootstrapping key's 58-bit grid with the GLWE noise, as the re-key key:
 *   mask-digit row l = 0, 1:  m = bit x (-S) x 2^(64 - 16 (l + 1));     body-digit row l:  m = bit x 2^(64 - 16 (l + 1)).
 * 128 KB per bit.  Randomness follows the re-key key's rule: a ChaCha20 key drawn from getrandom(2) for that call alone
 * (streams = the row number, domains 2 = masks / 3 = noise); an insecure seeded client derives it from its seed, a tag of
 * its own and the number of queries it has made so far (tests only).  Two queries, also for the same index, never share
 * a mask or noise.
 * NOISE AND BOOKKEEPING (host side; a planner context does all of it and allocates nothing).  One CMux adds the external
 * product's sigma 2^33.1 and a 32-bit rounding's 2^35.2: variance 1.03 x one re-key's, charged as FHS_SELECT_REKEY_COST
 * re-keys.  The result's re-key counter is the source's + FHS_SELECT_REKEY_COST x (tree levels + rotate bits); a result
 * past FHS_STORE_MAX_REKEYS is refused with FHS_ERR_LIMIT before anything is allocated.  Block j of the result takes the
 * maximum figure and the maximum `cycles` of block j over all R rows; its rotation group is 0 if no candidate block of
 * any row has one, otherwise ONE fresh group shared by all such result blocks (fully correlated: the upper bound). */
#define FHS_SELECT_MAX_ROW_CHARS 512
#define FHS_SELECT_QUERY_BIT_WORDS ((size_t)4 * 2 * 2048)        /* u64 words of one index bit's GGSW */
#define FHS_SELECT_QUERY_WORDS(bits) ((size_t)(bits) * FHS_SELECT_QUERY_BIT_WORDS)
#define FHS_SELECT_REKEY_COST 2
/* ceil(log2(n_chars / row_chars)), or 0 for a shape fhs_store_select refuses. */
int fhs_store_select_bits(size_t n_chars, size_t row_chars);
/* A fresh query for row `index` (bit k of it goes into GGSW k; bits of index above `bits` are ignored).  bits 1..24. */
int fhs_client_select_query(fhs_client *ck, uint64_t index, int bits, uint64_t *query_out /*[FHS_SELECT_QUERY_WORDS(bits)]*/);
/* Selects the row.  The query crosses the bus as it is through the pinned staging buffer and is converted to the
 * transform domain on the device (one launch); one kernel launch per tree level and per rotate bit on the context's stream, behind every queued
 * fhs_store_get / fhs_store_rekey of the entry; *id_out receives the new entry.  Needs no server key loaded at the time
 * of the call, but the transform tables that the FIRST fhs_load_server_key of a context uploads: FHS_ERR_STATE before
 * that on a device context (a later server-key reload changes nothing).  FHS_ERR_ARG: unknown id, a refused shape, bits
 * != fhs_store_select_bits.  FHS_ERR_LIMIT: see above. */
int fhs_store_select(fhs_ctx *ctx, uint64_t id, size_t row_chars, const uint64_t *query, int bits, uint64_t *id_out);
/* Host reference (public data only, no GPU): the same words as the device.  mask32 / body32: the WHOLE entry as
 * fhs_store_export gives it, n_blocks_entry = 4 x its characters; mask32_out[2048], body32_out[4 row_chars]. */
int fhs_store_select_host(const uint64_t *query, int bits, const void *mask32, const void *body32, size_t n_blocks_entry,
                          size_t row_chars, void *mask32_out, void *body32_out);
/* Diagnostic: the device kernels on raw words, the arguments of fhs_store_select_host.  FHS_ERR_STATE on a planner
 * context or before the first server key. */
int fhs_debug_select_device(fhs_ctx *ctx, const uint64_t *query, int bits, const void *mask32, const void *body32,
                            size_t n_blocks, size_t row_chars, void *mask32_out, void *body32_out);

/* ---- string store: seeded queries, queries converted on the GPU, several queries per call -------------------
 *   Nothing above changes: the full-form query, fhs_store_select and the host reference keep
 * their words.
 * THE SEEDED QUERY is the query above with the mask of every GGSW row drawn from a PUBLIC 256-bit seed, so only the
 * bodies travel: 64 KB per index bit instead of 128 KB, plus 32 bytes.  It follows the seeded-stream convention of
 * "compressed ciphertexts and server keys":
 *   select query, index bit k, GGSW row r      domain 8, stream 4k + r   draws 0..2047, each & ~63 (the 58-bit grid)
 *                                                                        = the row's mask polynomial; the row's body
 *                                                                        polynomial is sent
 * Row r of bit k carries the message and the shift of the full form's row.  THE NOISE NEVER COMES FROM THE SEED: the seed
 * is public, so the noise is drawn from the client's SECRET generator key, noise streams 2^63 + 2^62 + (call << 7) +
 * 4k + r, a range no other object of the client draws from, distinct per call, bit and row.  The seed is OS entropy; an
 * insecure seeded client derives it from its 64-bit seed, a tag of its own and the number of SEEDED queries it has made
 * (a counter of its own: seeded queries do not move what fhs_client_select_query returns next).
 * fhs_expand_select_query (public data only) rebuilds the full form, [bit][row][mask, body][2048]: everything that
 * takes a full-form query, fhs_store_select_host included, takes the expansion.
 * ON THE DEVICE the query -- either form -- crosses the bus as it is and select_query_to_ntt_kernel converts it to the
 * transform domain; the masks of a seeded query are regenerated inside that kernel.  fhs_store_select_seeded gives word
 * for word what fhs_store_select gives on the expansion.
 * SEVERAL QUERIES PER CALL.  fhs_store_select_batch runs n queries (all of one form, all for the same entry and
 * row_chars) through ONE conversion launch and one CMux launch per tree level and per rotate bit, whatever n is.  Result
 * i is word for word what fhs_store_select gives for query i alone, with bookkeeping of its own (figures, cycles, its own
 * fresh rotation group, re-key counter); ids_out are consecutive, in the order of the queries.  The call is ATOMIC: an
 * unknown id, a refused shape, bits != fhs_store_select_bits, n = 0 or n > FHS_SELECT_MAX_BATCH, a NULL pointer
 * (FHS_ERR_ARG), the re-key counter limit or a workspace above FHS_SELECT_BATCH_MAX_BYTES (FHS_ERR_LIMIT) create
 * nothing and write 0 to every ids_out.  The workspace is what the context keeps for the call: the n converted queries
 * (n x bits x 8 polynomials x 2 primes x 2048 doubles) and the two buffers the tree's levels alternate between
 * (n x (max(1, ceil(G / 2)) + max(1, ceil(G / 4))) GLWEs of 32-bit words); fhs_store_select_batch_bytes reports it, 0
 * for a refused shape or n. */
#define FHS_DOM_SEEDED_SELECT 8
#define FHS_SELECT_SEEDED_BIT_WORDS ((size_t)4 * 2048)          /* body words of one index bit */
#define FHS_SELECT_SEEDED_WORDS(bits) ((size_t)(bits) * FHS_SELECT_SEEDED_BIT_WORDS)
#define FHS_SELECT_FORM_FULL 0
#define FHS_SELECT_FORM_SEEDED 1
#define FHS_SELECT_MAX_BATCH 64
#define FHS_SELECT_BATCH_MAX_BYTES ((size_t)256 * 1024 * 1024)
/* A fresh seeded query for row `index`: seed_out and bodies[bits][4][2048].  bits 1..24. */
int fhs_client_select_query_seeded(fhs_client *ck, uint64_t index, int bits, uint32_t seed_out[8],
                                   uint64_t *bodies /*[FHS_SELECT_SEEDED_WORDS(bits)]*/);
/* Public data only: the full form of a seeded query. */
int fhs_expand_select_query(const uint32_t seed[8], const uint64_t *bodies, int bits,
                            uint64_t *query_out /*[FHS_SELECT_QUERY_WORDS(bits)]*/);
/* fhs_store_select with a seeded query. */
int fhs_store_select_seeded(fhs_ctx *ctx, uint64_t id, size_t row_chars, const uint32_t seed[8], const uint64_t *bodies,
                            int bits, uint64_t *id_out);
/* n queries of one form: queries[i] points at the full words (FHS_SELECT_FORM_FULL; seeds is NULL) or at the bodies
 * (FHS_SELECT_FORM_SEEDED; seeds[i][8] is its seed). */
int fhs_store_select_batch(fhs_ctx *ctx, uint64_t id, size_t row_chars, int form, const uint32_t *seeds,
                           const uint64_t *const *queries, size_t n, int bits, uint64_t *ids_out /*[n]*/);
size_t fhs_store_select_batch_bytes(size_t n_chars, size_t row_chars, size_t n);
/* Diagnostic: select_query_to_ntt_kernel alone.  form FULL: words = the query, seed ignored; form SEEDED: words = the
 * bodies.  out[bits][8 polynomials][2 primes][2048] doubles, the transform-domain layout of the CMux kernel.
 * FHS_ERR_STATE on a planner context or before the first server key. */
int fhs_debug_select_query_device(fhs_ctx *ctx, int form, const uint32_t seed[8], const uint64_t *words, int bits,
                                  double *out);
/* Host reference of that conversion (the routine the key loads use): the same doubles, bit for bit. */
int fhs_select_query_ntt_host(const uint64_t *query, int bits, double *out);
/* Diagnostic: fhs_debug_select_device with a seeded query. */
int fhs_debug_select_seeded_device(fhs_ctx *ctx, const uint32_t seed[8], const uint64_t *bodies, int bits,
                                   const void *mask32, const void *body32, size_t n_blocks, size_t row_chars,
                                   void *mask32_out, void *body32_out);

/* ---- block pool: what it holds, and giving it back ---------------------------------------------------------
 * Ciphertext blocks are carved from chunks of 2048 blocks (2048 x 2050 x 8 = 33 587 200 B each).  A released block goes
 * back to the context's free list, its chunk stays: without a trim a context sits on the high-water mark of its blocks
 * until it is destroyed, however little of it is live (a parked 4097-character string: 268 MB held for 139 KB in use).
 * Nothing below happens unless it is called; allocation order and results are otherwise unchanged.
 * A planner context holds no chunk: stats report the live blocks and zeros for chunks, free blocks and bytes, and a trim
 * flushes, moves nothing and releases nothing. */
/* out[0] chunks held, out[1] blocks per chunk (2048), out[2] live blocks, out[3] free blocks (reusable now),
 * out[4] blocks freed under a scheduled tick and not reusable yet, out[5] device bytes of the chunks */
int fhs_pool_stats(fhs_ctx *ctx, uint64_t out[6]);
/* fhs_pool_trim flushes first, as every download does (all scheduled ticks of fhs_submit are drained), and then keeps
 * K = ceil((live + keep_free_blocks) / 2048) chunks: keep_free_blocks is the room left for the next request without a
 * new allocation.  FHS_TRIM_RELEASE gives back chunks that hold no live block, as many as exceed K.  FHS_TRIM_COMPACT
 * takes as victims the (chunks - K) chunks with the fewest live blocks -- ties go to the chunk allocated last -- copies
 * every live block of a victim into a free slot of a kept chunk on the GPU (one kernel launch per 2048 blocks; only
 * the pointer tables cross the bus), waits for the stream and gives the victims back.  A moved block is the same block
 * at another address: handles, figures, rotation groups and packing counts are untouched.  *blocks_moved /
 * *bytes_released (either may be NULL) receive what was done; a trim with nothing to give back is not an error.
 * FHS_ERR_ARG: a null context or an unknown mode.  FHS_ERR_STATE: levels planned by fhs_flush_plan are still waiting for
 * fhs_flush_level_commit (nothing is flushed or changed), or the flush itself failed.  In level-parallel mode the flush
 * is collective: every rank trims at the same point or none does. */
#define FHS_TRIM_RELEASE 0   /* give back the chunks that hold no live block; moves nothing */
#define FHS_TRIM_COMPACT 1   /* first move live blocks out of the emptiest chunks, then release */
int fhs_pool_trim(fhs_ctx *ctx, int mode, size_t keep_free_blocks, uint64_t *blocks_moved /*may be NULL*/,
                  uint64_t *bytes_released /*may be NULL*/);
/* The victim choice of FHS_TRIM_COMPACT alone, a pure host function: live_per_chunk[n_chunks] in allocation order (each
 * <= 2048, else FHS_ERR_ARG) -> victim_out[i] = 1 for the chunks a compacting trim would give back, 0 for the kept. */
int fhs_debug_pool_plan(const uint32_t *live_per_chunk, size_t n_chunks, size_t keep_free_blocks,
                        uint8_t *victim_out /*[n_chunks]*/);

#ifdef __cplusplus
}
#endif
#endif
