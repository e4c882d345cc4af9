// Host runtime: device context, key material, batched-PBS dispatch, kernel timing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fhestring_hip.h"
#include "dist.h"
#include "fft_tables.h"
#include "hip_owners.h"
#include "ntt_tables.h"
#include "pbs_kernels.h"

namespace fhs {

// the arithmetics fhs_set_arithmetic selects (FHS_ARITH_*, include/fhestring_hip.h)
constexpr int N_ARITH = 4;
constexpr bool is_f64_fft(int arith) { return arith == FHS_ARITH_F64_FFT || arith == FHS_ARITH_F64_FFT_MB2; }

// where build_fft_key() put the f64-FFT tables inside Context::d_fft_tables
struct FftTablePtrs {
    const double *lanetab = nullptr;   // [12][64]
    const double *weff = nullptr;      // [1024][2]
    const double *mono = nullptr;      // [4096][2]
    const double *r16 = nullptr;       // [16][2]
};

// HIP-event timing of the two PBS kernels on the stream they are launched on
struct KernelTimer {
    struct Pending { Event e0, e1; int kind; uint64_t units; uint32_t launches; bool shifted_acc; };
    std::vector<Pending> pending;
    std::vector<Event> pool;         // resolved events wait here for the next launch; they go with the timer
    // 0 = blind rotation (exact NTT kernel, or the 2-wavefront FFT kernel), 1 = keyswitch,
    // 2 = blind rotation on the 4-wavefront FFT kernel (batches <= fft4_max_batch),
    // 3 = the part of kind 0 that ran the shifted-accumulator instantiation of the 2-wavefront FFT kernel (counted twice)
    static constexpr int KINDS = 4;
    double ms[KINDS] = {};
    uint64_t n[KINDS] = {};          // KERNEL launches covered (a blind rotation cut into one-round launches counts each of them:
                                     // the per-launch average then is what `rocprofv3 --kernel-trace --stats` reports per kernel)
    uint64_t units[KINDS] = {};      // PBS covered by the timed launches
    bool enabled = true;
    Event get();
    void begin(int kind, uint64_t units, hipStream_t s, bool shifted_acc = false);
    void end(hipStream_t s, uint32_t kernel_launches = 1);
    void resolve();   // synchronises pending events and accumulates
    void reset();
};

class Context {
  public:
    int device = 0;
    Stream stream;                   // declared before every buffer: the buffers go first, then the stream
    std::string err;
    bool key_loaded = false;

    // key material on device: every allocation has one owner, and a key is loaded exactly when its owner holds memory
    DevBuf d_ksk_planes;             // int8: KSK as 8 byte planes in MFMA fragment order (ks_kernels.hip)
    DevBuf d_bsk_ntt;                // double
    DevBuf d_tables;                 // double: fwd_uni | fwd_lane | inv_uni | inv_lane | mono
    NttTables tw{};                  // ... and where they landed
    double crt_c = 0;

    // the selected arithmetic, FHS_ARITH_* (default: exact two-prime NTT).  The server key may be loaded before or after
    // an f64-FFT arithmetic is selected: the Fourier-domain key is built from the retained standard-domain key by whichever
    // comes second (install_server_key / set_arithmetic -> build_fft_key).
    int arith = FHS_ARITH_EXACT_NTT;
    DevBuf d_bsk_fft;                // double: Fourier-domain key of FHS_ARITH_F64_FFT (fft_kernels.hip, fft4_kernels.hip)
    DevBuf d_bsk_std;                // uint64: standard-domain key, kept for a later conversion to the Fourier domain
    DevBuf d_fft_tables;             // double: lanetab | weff | mono | r16
    FftTablePtrs ft;                 // ... and where they landed
    DevBuf d_work_counter;           // uint32: persistent-workgroup ciphertext counter of the 2-wavefront FFT kernel (64 B)
    int wg_slots = 1024;                  // 4 workgroups per CU
    // pair keys of the two-key-bits-per-product arithmetics; they belong to the server key they were generated with
    DevBuf d_bsk_mb;                 // double, FHS_ARITH_F64_FFT_MB2 (fftmb_kernels.hip): [371][K1,K2,K3][4][1024] complex
    DevBuf d_bsk_ntt_mb;             // double, FHS_ARITH_EXACT_NTT_MB2: [371][K1,K2,K3][4][2 primes][2048] residues
    const double *d_ntt_mono = nullptr;   // [2][4096] inside d_tables
    // packed result download (pack_kernels.hip): the 11 automorphism keyswitch keys as residues modulo the two NTT primes
    DevBuf d_pack_key_ntt;           // double: [11][3][2 cols][2 primes][2048]
    int load_packing_key(const uint64_t *key);   // [FHS_PACK_KEY_WORDS] u64 standard domain (fhs_client_packing_key)
    // string-store re-key (rekey_kernels.hip): the GLWE keyswitch key S_old -> S_new as residues, an auxiliary key like the
    // packing key (dropped by a server-key reload)
    DevBuf d_rekey_key_ntt;          // double: [2][2 cols][2 primes][2048]
    int load_rekey_key(const uint64_t *key);     // [FHS_REKEY_KEY_WORDS] u64 standard domain, or nullptr: unload
    // the conversion and upload behind both loaders (internal)
    int load_keyswitch_key(const uint64_t *key, size_t n_polys, DevBuf &d_key_ntt, const char *malloc_what, const char *copy_what,
                           hipError_t (*prepare)());
    int load_multibit_key(const uint64_t *bsk_mb2);   // [371][K1,K2,K3][4][2048] u64 standard domain (fhs_client_bsk_mb2)
    int fft4_max_batch = 512;                // batches up to this size use the 4-wavefront kernel (lower latency)
    size_t launch_chunk[N_ARITH] = {};       // per arithmetic: ciphertexts per blind-rotation launch (0 = whole batch)
    int set_arithmetic(int mode);
    // keyswitch of a dense batch into ks_buf (timed as kernel kind 1); ks_buf must hold B rows
    int keyswitch(const uint64_t *d_in, size_t B, hipStream_t s);
    // blind rotation in the selected arithmetic (timed as kernel kind 0)
    // luts_clean: the low 8 bits of every word of the tables under d_luts are zero (luts_low_bytes_clear, taken when the
    // tables were uploaded; false where nobody looked, e.g. a caller's device pointer): the 2-wavefront FFT kernel then runs
    // its shifted-accumulator instantiation, timed as kernel kind 3 beside kind 0
    int blind_rotate(const uint64_t *d_ks, const uint32_t *d_lut_idx, const uint64_t *d_luts, bool luts_clean, uint64_t *d_out,
                     uint64_t *const *d_out_ptrs, size_t B, hipStream_t s, uint64_t *const *d_body_ptrs = nullptr);
    static bool luts_low_bytes_clear(const uint64_t *luts, size_t n_words);

    // multi-GPU exchange (fhs_dist_init): RCCL communicator of this context, or a host transport
    Dist dist;
    DevBuf xchg_send, xchg_recv;     // char exchange of the sharded string ops / level slices of the level-parallel flush

    // scratch
    DevBuf dig_buf;                  // keyswitch digits of the current batch
    DevBuf ks_buf, ms_buf, in_buf, out_buf, lutidx_buf, luts_buf, tab_buf;
    DevBuf pack_ws[2], pack_tab, pack_out;   // packing: ping-pong tree levels, leaf table, u16 result (allocated on first use, kept)
    // select by encrypted index (select_kernels.hip), allocated on first use and kept, grow-only: the queries of a call
    // as residues [queries][bits][4][2 cols][2 primes][2048], written by select_query_to_ntt_kernel, and the two buffers
    // the tree's levels alternate between, ceil(G / 2) and ceil(G / 4) GLWEs of 32-bit words per query for the largest
    // (queries x entry of G groups) so far
    DevBuf sel_query, sel_ws[2];
    bool select_prepared = false;    // prepare_device_for_select has run on this device
    KernelTimer timer;

    int init(int device_id);
    ~Context();                      // waits for the stream, closes the exchange, resolves the timer; then the members go
    int fail(int code, const std::string &msg) { err = msg; return code; }
    int hip_fail(hipError_t e, const char *what);

    int load_server_key(const uint64_t *bsk, const uint64_t *ksk);
    // seeded masks expanded on the device (fhs_load_compressed_server_key), then the same tail as load_server_key
    int load_compressed_server_key(const uint32_t seed[8], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies);
    int install_server_key(const uint64_t *bsk, const uint64_t *d_ksk);
    int build_fft_key();
    // all device pointers; enqueues KS+MS then blind rotation on `s`.  luts_clean as for blind_rotate: nobody has looked at
    // a caller's device tables, so the C entry point leaves it false
    int pbs_batch_device(const uint64_t *d_in, const uint32_t *d_lut_idx, const uint64_t *d_luts,
                         uint64_t *d_out, size_t B, hipStream_t s, bool luts_clean = false);
    int pbs_batch_shifted_host(const uint64_t *in, const uint32_t *lut_idx, const uint64_t *luts, size_t n_luts,
                               const uint32_t *shifts, size_t S, uint64_t *out, size_t B);
    int pbs_batch_host(const uint64_t *in, const uint32_t *lut_idx, const uint64_t *luts, size_t n_luts,
                       uint64_t *out, size_t B);
    int ks_ms_batch_host(const uint64_t *in, uint32_t *ms_out, size_t B);
    int blind_rotate_host(const uint64_t *ks, const uint32_t *lut_idx, const uint64_t *luts, size_t n_luts,
                          uint64_t *out, size_t B);
};

}  // namespace fhs
