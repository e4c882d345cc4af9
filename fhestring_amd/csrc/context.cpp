#include "context.h"
#include "pack_kernels.h"
#include "rekey_kernels.h"
#include "seeded_kernels.h"
#include "../../include/fhestring_hip.h"

#include <algorithm>
#include <cstdlib>
#include <utility>

namespace fhs {

namespace {
constexpr size_t KSK_BYTES = (size_t)BIG_N * KS_LEVEL * SMALL_CT * sizeof(uint64_t);
constexpr size_t BSK_BYTES = (size_t)LWE_N * 4 * POLY_N * sizeof(uint64_t);
}  // namespace

#define HIP_TRY(expr, what)                                \
    do {                                                   \
        hipError_t e__ = (expr);                           \
        if (e__ != hipSuccess) return hip_fail(e__, what); \
    } while (0)

Event KernelTimer::get() {
    if (pool.empty()) return Event();
    Event e = std::move(pool.back());
    pool.pop_back();
    return e;
}
void KernelTimer::begin(int kind, uint64_t u, hipStream_t s, bool shifted_acc) {
    if (!enabled) return;
    if (pending.size() > 4096) resolve();
    Pending p{get(), get(), kind, u, 1, shifted_acc};
    (void)hipEventRecord(p.e0.get(), s);
    pending.push_back(std::move(p));
}
void KernelTimer::end(hipStream_t s, uint32_t kernel_launches) {
    if (!enabled || pending.empty()) return;
    pending.back().launches = kernel_launches ? kernel_launches : 1;
    (void)hipEventRecord(pending.back().e1.get(), s);
}
void KernelTimer::resolve() {
    for (auto &p : pending) {
        (void)hipEventSynchronize(p.e1.peek());
        float t = 0;
        if (hipEventElapsedTime(&t, p.e0.peek(), p.e1.peek()) == hipSuccess) {
            for (int k : {p.kind, 3}) {
                ms[k] += t;
                n[k] += p.launches;
                units[k] += p.units;
                if (!p.shifted_acc) break;
            }
        }
        pool.push_back(std::move(p.e0));
        pool.push_back(std::move(p.e1));
    }
    pending.clear();
}
void KernelTimer::reset() {
    resolve();
    for (int k = 0; k < KINDS; k++) { ms[k] = 0; n[k] = 0; units[k] = 0; }
}
int Context::hip_fail(hipError_t e, const char *what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return -2;
}

int Context::init(int device_id) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(-2, "no HIP device visible: this backend has no CPU fallback");
    if (device_id < 0 || device_id >= n) return fail(-1, "device_id out of range");
    device = device_id;
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(-2, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    HIP_TRY(prepare_device_for_kernels(), "hipFuncSetAttribute (dynamic LDS)");
    HIP_TRY(prepare_device_for_fft4(), "hipFuncSetAttribute (dynamic LDS, 4-wavefront kernel)");
    HIP_TRY(prepare_device_for_keyswitch(), "hipFuncSetAttribute (dynamic LDS, wide keyswitch kernel)");
    // FHS_STREAM_CU_MASK=<hex word>[,<hex word>...] (32 CUs per word, lowest CUs first): this context's stream only
    // runs on the compute units of the mask (hipExtStreamCreateWithCUMask) and the persistent kernels size their grid for
    // them.  An experiment switch (tools/exp_cumask.py, DESIGN.md section 5d: a narrow dependency level of one request on
    // a slice of the chip beside another request's wide level), not a tuning knob of the product.
    int cus = prop.multiProcessorCount;
    if (const char *m = std::getenv("FHS_STREAM_CU_MASK")) {
        std::vector<uint32_t> mask;
        int bits = 0;
        for (const char *q = m; *q;) {
            char *end = nullptr;
            const unsigned long w = std::strtoul(q, &end, 16);
            if (end == q) break;
            mask.push_back((uint32_t)w);
            bits += __builtin_popcount((uint32_t)w);
            q = *end == ',' ? end + 1 : end;
            if (*end != ',') break;
        }
        if (mask.empty() || bits == 0 || bits > cus) return fail(-1, "FHS_STREAM_CU_MASK: expected hex words selecting 1.." + std::to_string(cus) + " CUs");
        HIP_TRY(stream.create(mask.data(), (uint32_t)mask.size()), "hipExtStreamCreateWithCUMask");
        cus = bits;
    } else {
        HIP_TRY(stream.create(), "hipStreamCreate");
    }
    wg_slots = 4 * cus;
    // two-bit f64 kernel: one round of resident workgroups per launch (its 73 MB key only stays inside the L2 window
    // while the workgroups walk it together; consecutive launches overlap at the seams): 202 k instead of 183 k PBS/s at
    // 4096 rows, 214 k instead of 152 k at 14 336.  The classic f64 kernel (48 MB key) does not care below 4096 rows.
    launch_chunk[FHS_ARITH_F64_FFT_MB2] = (size_t)wg_slots;
    // classic f64 kernel (round 5): one round per launch as well.  Time-neutral (default bench 134.5 k PBS/s plain, 135.5 k
    // chunked; 3968-wide launches 30.12 ms plain, 30.33 ms chunked: profiles/r05_chunk_ab.txt) but every launch restarts
    // the key walk of all workgroups together: L2 hit rate 95 -> 98.5 %, fabric-side traffic 6.3 -> 2.4 GB per launch
    // group -- traffic that eight processes on one node would otherwise multiply by eight.  A remainder below a quarter of
    // a round rides in the last launch instead of becoming one of its own (blind_rotate()).
    launch_chunk[FHS_ARITH_F64_FFT] = (size_t)wg_slots;
    HIP_TRY(d_work_counter.reserve_exact(64), "hipMalloc counter");
    return 0;
}

Context::~Context() {
    if (stream) (void)hipStreamSynchronize(stream);
    dist.shutdown();
    timer.resolve();
}

int Context::load_server_key(const uint64_t *bsk, const uint64_t *ksk) {
    if (!bsk || !ksk) return fail(-1, "null key pointer");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    DevBuf d_ksk;
    HIP_TRY(d_ksk.reserve_exact(KSK_BYTES), "hipMalloc ksk staging");
    hipError_t e = hipMemcpy(d_ksk.ptr, ksk, KSK_BYTES, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_bsk_std.reserve_exact(BSK_BYTES);
    if (e == hipSuccess) e = hipMemcpy(d_bsk_std.ptr, bsk, BSK_BYTES, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "copy server key");
    return install_server_key(bsk, d_ksk.as<uint64_t>());
}

// Compressed server key: the masks are regenerated on the device from the public seed (seeded_kernels.hip) into the
// standard-domain BSK and a KSK staging buffer; the exact arithmetic's key is converted on the host from a read-back copy.
int Context::load_compressed_server_key(const uint32_t seed[8], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies) {
    if (!seed || !bsk_bodies || !ksk_bodies) return fail(-1, "null key pointer");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    SeedKey key;
    for (int i = 0; i < 8; i++) key.w[i] = seed[i];
    const size_t bb = FHS_CBSK_BODY_WORDS * 8, kb = FHS_CKSK_BODY_WORDS * 8;
    DevBuf d_ksk;
    std::vector<uint64_t> bsk((size_t)LWE_N * 4 * POLY_N);
    {
        DevBuf d_bodies;
        hipError_t e = d_ksk.reserve_exact(KSK_BYTES);
        if (e == hipSuccess) e = d_bodies.reserve_exact(bb + kb);
        if (e == hipSuccess) e = d_bsk_std.reserve_exact(BSK_BYTES);
        uint64_t *const bodies = d_bodies.as<uint64_t>();
        if (e == hipSuccess) e = hipMemcpy(bodies, bsk_bodies, bb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(bodies + FHS_CBSK_BODY_WORDS, ksk_bodies, kb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_expand_seeded_bsk(key, bodies, d_bsk_std.as<uint64_t>(), stream);
        if (e == hipSuccess) e = launch_expand_seeded_ksk(key, bodies + FHS_CBSK_BODY_WORDS, d_ksk.as<uint64_t>(), stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = hipMemcpy(bsk.data(), d_bsk_std.ptr, BSK_BYTES, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "compressed server key expansion");
    }
    return install_server_key(bsk.data(), d_ksk.as<uint64_t>());
}

// The shared tail of both key loads: d_bsk_std holds the standard-domain BSK (`bsk`: a host copy of it), d_ksk the KSK.
int Context::install_server_key(const uint64_t *bsk, const uint64_t *d_ksk) {
    // what was derived from the previous server key, or generated with it, goes with it: the Fourier-domain key (rebuilt
    // below from the new standard-domain key if an f64-FFT arithmetic is selected, otherwise the first time one is), both
    // pair keys, the packing key and the re-key key (one rule for auxiliary keys)
    for (DevBuf *b : {&d_bsk_fft, &d_bsk_mb, &d_bsk_ntt_mb, &d_pack_key_ntt, &d_rekey_key_ntt}) b->release();
    const size_t bsk_ntt_doubles = (size_t)LWE_N * 4 * 2 * POLY_N;
    HIP_TRY(d_bsk_ntt.reserve_exact(bsk_ntt_doubles * sizeof(double)), "hipMalloc bsk");
    {   // the KSK is only kept as byte planes in MFMA fragment order (ks_kernels.hip)
        hipError_t e = d_ksk_planes.reserve_exact(ks_planes_bytes());
        if (e == hipSuccess) e = launch_ksk_to_planes(d_ksk, d_ksk_planes.as<int8_t>(), stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        HIP_TRY(e, "ksk -> byte planes");
    }
    {
        std::vector<double> host(bsk_ntt_doubles);
        convert_bsk_to_ntt(bsk, host.data());
        HIP_TRY(hipMemcpy(d_bsk_ntt.ptr, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice),
                "copy bsk");
    }
    HostNttTables ht;
    build_ntt_tables(ht);
    const size_t n_tab = ht.fwd_uni.size() + ht.fwd_lane.size() + ht.inv_uni.size() + ht.inv_lane.size() + ht.mono.size();
    HIP_TRY(d_tables.reserve_exact(n_tab * sizeof(double)), "hipMalloc tables");
    double *pd = d_tables.as<double>();
    auto up = [&](const std::vector<double> &v, const double *&slot) -> hipError_t {
        slot = pd;
        hipError_t e = hipMemcpy(pd, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice);
        pd += v.size();
        return e;
    };
    HIP_TRY(up(ht.fwd_uni, tw.fwd_uni), "copy tables");
    HIP_TRY(up(ht.fwd_lane, tw.fwd_lane), "copy tables");
    HIP_TRY(up(ht.inv_uni, tw.inv_uni), "copy tables");
    HIP_TRY(up(ht.inv_lane, tw.inv_lane), "copy tables");
    HIP_TRY(up(ht.mono, d_ntt_mono), "copy tables");
    crt_c = ht.crt_c;
    {   // the kernel's baked-in uniform twiddles must equal the exactly derived ones
        std::vector<double> fu(64), iu(128);
        double c = 0;
        HIP_TRY(read_device_ntt_consts(fu.data(), iu.data(), &c), "read device constants");
        if (fu != ht.fwd_uni || iu != ht.inv_uni || c != ht.crt_c)
            return fail(-3, "ntt_consts.inc does not match the derived twiddle tables (regenerate it)");
    }
    // the standard-domain key stays on the device (48.6 MB of 288 GB): the Fourier-domain key is built from it with the
    // device's own forward transform -- now if the f64 arithmetic is selected, otherwise the first time it is
    if (is_f64_fft(arith))
        if (int rc = build_fft_key()) return rc;
    key_loaded = true;
    return 0;
}

// Fourier-domain bootstrapping key of the f64 arithmetics from the retained standard-domain key (load_server_key, or the
// first fhs_set_arithmetic(FHS_ARITH_F64_FFT) after a key was loaded under the exact arithmetic: either order works).
int Context::build_fft_key() {
    if (!d_bsk_std) return fail(-3, "server key not loaded");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    HostFftTables ht;
    build_fft_tables(ht);
    {   // the kernel's literal twiddles must equal the libm-derived ones
        double wr[16], wi[16], ur[3], ui[3];
        fft_uniform_consts(wr, wi, ur, ui);
        bool ok = true;
        for (int k = 1; k < 16; k++) ok = ok && wr[k] == ht.w_re[k] && wi[k] == ht.w_im[k];
        for (int k = 0; k < 3; k++) ok = ok && ur[k] == ht.u_re[k] && ui[k] == ht.u_im[k];
        if (!ok) return fail(-3, "fft_consts.inc does not match the libm-derived twiddles (regenerate it)");
    }
    std::vector<double> flat;                      // one upload; every table keeps the pointer to where it landed
    auto put = [&](const std::vector<double> &v) {
        const size_t at = flat.size();
        flat.insert(flat.end(), v.begin(), v.end());
        return at;
    };
    const size_t at_lanetab = put(ht.lanetab), at_weff = put(ht.weff), at_mono = put(ht.mono), at_r16 = put(ht.r16);
    HIP_TRY(d_fft_tables.reserve_exact(flat.size() * sizeof(double)), "hipMalloc fft tables");
    HIP_TRY(hipMemcpy(d_fft_tables.ptr, flat.data(), flat.size() * sizeof(double), hipMemcpyHostToDevice), "copy fft tables");
    const double *const tab = d_fft_tables.as<double>();
    ft.lanetab = tab + at_lanetab; ft.weff = tab + at_weff; ft.mono = tab + at_mono; ft.r16 = tab + at_r16;
    const size_t n = (size_t)LWE_N * 4 * POLY_N;   // 1024 complex (2048 doubles) per polynomial
    HIP_TRY(d_bsk_fft.reserve_exact(n * sizeof(double)), "hipMalloc bsk fft");
    hipError_t e = launch_bsk_to_fft(d_bsk_std.as<uint64_t>(), d_bsk_fft.as<double>(), ft.lanetab, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) d_bsk_fft.release();      // not loaded
    HIP_TRY(e, "bsk -> Fourier domain");
    return 0;
}

int Context::keyswitch(const uint64_t *d_in, size_t B, hipStream_t s) {
    if (dig_buf.cap < ks_digits_bytes((int)B)) {
        HIP_TRY(hipStreamSynchronize(s), "sync");
        HIP_TRY(dig_buf.reserve(ks_digits_bytes((int)B)), "hipMalloc digits");
    }
    timer.begin(1, B, s);
    hipError_t e = launch_keyswitch_mfma(d_in, d_ksk_planes.as<int8_t>(), dig_buf.as<int8_t>(), ks_buf.as<uint64_t>(), (int)B, s,
                                         wg_slots / 4);
    timer.end(s);
    if (e != hipSuccess) return hip_fail(e, "keyswitch launch");
    return 0;
}

int Context::set_arithmetic(int mode) {
    if (mode < 0 || mode >= N_ARITH) return fail(-1, "unknown arithmetic mode");
    if (is_f64_fft(mode) && key_loaded && !d_bsk_fft)              // the key was loaded under the exact arithmetic: build
        if (int rc = build_fft_key()) return rc;                   // its Fourier-domain form now (either order works)
    if (mode == FHS_ARITH_F64_FFT_MB2 && key_loaded && !d_bsk_mb)
        return fail(-3, "the two-bits-per-product arithmetic needs the pair key in the Fourier domain: call "
                        "fhs_load_multibit_key while arithmetic 1 (f64 FFT) is selected, then fhs_set_arithmetic 2");
    if (mode == FHS_ARITH_EXACT_NTT_MB2 && key_loaded && !d_bsk_ntt_mb)
        return fail(-3, "the exact two-bits-per-product arithmetic needs the pair key converted to residues: call "
                        "fhs_load_multibit_key while the EXACT arithmetic (fhs_set_arithmetic 0) is selected, then "
                        "fhs_set_arithmetic 3");
    arith = mode;
    return 0;
}

// Pair key of the two-bits-per-product blind rotation: transformed with the device's own forward transform like the
// classic key (fftmb_kernels.hip).
int Context::load_multibit_key(const uint64_t *bsk_mb2) {
    if (!bsk_mb2) return fail(-1, "null key pointer");
    if (!key_loaded) return fail(-3, "load the server key before the pair key");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    if (!is_f64_fft(arith)) {
        // exact arithmetic: residues of the pair key modulo the two NTT primes, on the 57-bit torus grid (nttmb_kernels.hip)
        if (!ntt_slot_roots_are_bitreversed()) return fail(-3, "internal: NTT slot order is not bit-reversed");
        const size_t n_d = (size_t)(LWE_N / 2) * 3 * 4 * 2 * POLY_N;
        std::vector<double> host(n_d);
        convert_bsk_to_ntt(bsk_mb2, host.data(), (LWE_N / 2) * 3, 7);
        HIP_TRY(d_bsk_ntt_mb.reserve_exact(n_d * sizeof(double)), "hipMalloc pair key (NTT)");
        HIP_TRY(hipMemcpy(d_bsk_ntt_mb.ptr, host.data(), n_d * sizeof(double), hipMemcpyHostToDevice), "copy pair key");
        HIP_TRY(prepare_device_for_ntt_mb2(), "kernel attributes");
        return 0;
    }
    if (!d_fft_tables)
        return fail(-3, "load the server key in an f64-FFT arithmetic (fhs_set_arithmetic 1 or 2) before the pair key");
    const int n_polys = (LWE_N / 2) * 3 * 4;
    const size_t n = (size_t)n_polys * POLY_N;            // u64 in, doubles out (1024 complex per polynomial)
    DevBuf d_std;
    HIP_TRY(d_std.reserve_exact(n * sizeof(uint64_t)), "hipMalloc pair key staging");
    hipError_t e = d_bsk_mb.reserve_exact(n * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(d_std.ptr, bsk_mb2, n * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_bsk_to_fft(d_std.as<uint64_t>(), d_bsk_mb.as<double>(), ft.lanetab, stream, n_polys);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    HIP_TRY(e, "pair key -> Fourier domain");
    return 0;
}

// A GLWE keyswitch key (packing key, re-key key): converted on the host to the layout ntt_transform.h expects (both primes,
// 58-bit grid, 1/N folded in), exactly like the exact-arithmetic bootstrapping key, whatever arithmetic is selected.
int Context::load_keyswitch_key(const uint64_t *key, size_t n_polys, DevBuf &d_key_ntt, const char *malloc_what,
                                const char *copy_what, hipError_t (*prepare)()) {
    if (!ntt_slot_roots_are_bitreversed()) return fail(-3, "internal: NTT slot order is not bit-reversed");
    const size_t n_d = n_polys * 2 * POLY_N;
    std::vector<double> host(n_d);
    convert_polys_to_ntt(key, host.data(), n_polys, BSK_QUANT_BITS);
    HIP_TRY(hipStreamSynchronize(stream), "stream sync");     // a queued keyswitch may still read the previous key
    HIP_TRY(d_key_ntt.reserve_exact(n_d * sizeof(double)), malloc_what);
    HIP_TRY(hipMemcpy(d_key_ntt.ptr, host.data(), n_d * sizeof(double), hipMemcpyHostToDevice), copy_what);
    HIP_TRY(prepare(), "kernel attributes");
    return 0;
}

// Packing key: comes after the server key (whose load uploads the twiddle tables) and belongs to it.
int Context::load_packing_key(const uint64_t *key) {
    if (!key) return fail(-1, "null key pointer");
    if (!key_loaded) return fail(-3, "load the server key before the packing key");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    return load_keyswitch_key(key, PACK_KEY_POLYS, d_pack_key_ntt, "hipMalloc packing key", "copy packing key",
                              prepare_device_for_packing);
}

// Re-key key of the string store.  It has nothing to do with the server key but needs the twiddle tables its load
// uploads, and goes when the server key is replaced, like every auxiliary key.
int Context::load_rekey_key(const uint64_t *key) {
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    if (!key) {
        HIP_TRY(hipStreamSynchronize(stream), "stream sync");     // a queued re-key may still read it
        d_rekey_key_ntt.release();
        return 0;
    }
    if (!key_loaded) return fail(-3, "load the server key before the re-key key");
    return load_keyswitch_key(key, REKEY_KEY_POLYS, d_rekey_key_ntt, "hipMalloc re-key key", "copy re-key key",
                              prepare_device_for_rekey);
}

bool Context::luts_low_bytes_clear(const uint64_t *luts, size_t n_words) {
    uint64_t any = 0;
    for (size_t k = 0; k < n_words; k++) any |= luts[k];
    return (any & 0xFF) == 0;
}

int Context::blind_rotate(const uint64_t *d_ks, const uint32_t *d_lut_idx, const uint64_t *d_luts, bool luts_clean, uint64_t *d_out,
                          uint64_t *const *d_out_ptrs, size_t B, hipStream_t s, uint64_t *const *d_body_ptrs) {
    hipError_t e = hipSuccess;
    const bool four = arith == FHS_ARITH_F64_FFT && B <= (size_t)fft4_max_batch;
    if (arith == FHS_ARITH_F64_FFT_MB2 && !d_bsk_mb) return fail(-3, "pair key not loaded (fhs_load_multibit_key)");
    if (arith == FHS_ARITH_EXACT_NTT_MB2 && !d_bsk_ntt_mb)
        return fail(-3, "pair key not loaded in the exact arithmetic (fhs_load_multibit_key)");
    if (arith == FHS_ARITH_F64_FFT && !d_bsk_fft) return fail(-3, "Fourier-domain key not loaded");
    const bool shifted_acc = arith == FHS_ARITH_F64_FFT && !four && luts_clean;
    timer.begin(four ? 2 : 0, B, s, shifted_acc);
    // A launch is cut into chunks of launch_chunk[arith] ciphertexts (0 = whole batch): every chunk starts all workgroups on
    // the first key element together again.  The kernels whose key does not fit the L2 window of a drifting launch need
    // that (two-bit f64 kernel: 185 k PBS/s in launches of 3 072 - 4 096 rows, 144 k in one launch of 13 400).
    // A remainder of less than a quarter of a chunk does not become a launch of its own (8194 rows = 7 launches of 1024 and
    // one of 1026, not eight and a launch of 2 that costs a whole bootstrap alone).  The narrow-level kernel is never cut.
    const size_t chunk = (launch_chunk[arith] && !four) ? launch_chunk[arith] : B;
    uint32_t n_launches = 0;
    for (size_t off = 0, n = 0; off < B && e == hipSuccess; off += n) {
        n = std::min(chunk, B - off);
        if (B - off - n < chunk / 4) n = B - off;
        n_launches++;
        const uint64_t *ks = d_ks + off * SMALL_CT;
        const uint32_t *li = d_lut_idx + off;
        uint64_t *out = d_out ? d_out + off * BIG_CT : nullptr;
        uint64_t *const *outp = d_out_ptrs ? d_out_ptrs + off : nullptr;
        uint64_t *const *bodyp = d_body_ptrs ? d_body_ptrs + off : nullptr;   // rotation sharing (engine.cpp)
        if (arith == FHS_ARITH_EXACT_NTT_MB2) {
            BlindRotateNttMb2Params p{};
            p.ks = ks; p.lut_idx = li; p.luts = d_luts;
            p.bsk_ntt_mb = d_bsk_ntt_mb.as<double>(); p.tw = tw; p.crt_c = crt_c; p.mono = d_ntt_mono;
            p.out = out; p.out_ptrs = outp; p.body_ptrs = bodyp; p.B = (int)n;
            e = launch_blind_rotate_ntt_mb2(p, s);
        } else if (arith == FHS_ARITH_F64_FFT_MB2) {
            BlindRotateMb2Params p{};
            p.ks = ks; p.lut_idx = li; p.luts = d_luts;
            p.bsk_mb = d_bsk_mb.as<double>();
            p.lanetab = ft.lanetab; p.mono = ft.mono; p.r16 = ft.r16;
            p.work_counter = d_work_counter.as<uint32_t>();
            p.slots = wg_slots;
            p.out = out; p.out_ptrs = outp; p.body_ptrs = bodyp; p.B = (int)n;
            e = launch_blind_rotate_mb2(p, s);
        } else if (arith == FHS_ARITH_F64_FFT) {
            BlindRotateFftParams p{};
            p.ks = ks; p.lut_idx = li; p.luts = d_luts;
            p.bsk_fft = d_bsk_fft.as<double>();
            p.lanetab = ft.lanetab; p.weff = ft.weff;
            p.work_counter = d_work_counter.as<uint32_t>();
            p.slots = wg_slots;
            p.out = out; p.out_ptrs = outp; p.body_ptrs = bodyp; p.B = (int)n;
            e = four ? launch_blind_rotate_fft4(p, s) : launch_blind_rotate_fft(p, s, shifted_acc);
        } else {
            BlindRotateParams p{};
            p.ks = ks; p.lut_idx = li; p.luts = d_luts;
            p.bsk_ntt = d_bsk_ntt.as<double>(); p.tw = tw; p.crt_c = crt_c;
            p.out = out; p.out_ptrs = outp; p.body_ptrs = bodyp; p.B = (int)n;
            e = launch_blind_rotate(p, s);
        }
    }
    timer.end(s, n_launches);
    if (e != hipSuccess) return hip_fail(e, "blind_rotate launch");
    return 0;
}

int Context::pbs_batch_device(const uint64_t *d_in, const uint32_t *d_lut_idx, const uint64_t *d_luts,
                              uint64_t *d_out, size_t B, hipStream_t s, bool luts_clean) {
    if (!key_loaded) return fail(-3, "server key not loaded");
    if (B == 0) return 0;
    if (B > (size_t)1 << 24) return fail(-1, "batch too large");
    HIP_TRY(ks_buf.reserve(B * SMALL_CT * sizeof(uint64_t)), "hipMalloc ks");
    if (int rc = keyswitch(d_in, B, s)) return rc;
    if (int rc = blind_rotate(ks_buf.as<uint64_t>(), d_lut_idx, d_luts, luts_clean, d_out, nullptr, B, s)) return rc;
    return 0;
}

int Context::pbs_batch_host(const uint64_t *in, const uint32_t *lut_idx, const uint64_t *luts, size_t n_luts,
                            uint64_t *out, size_t B) {
    if (!in || !lut_idx || !luts || !out) return fail(-1, "null pointer");
    if (B == 0) return 0;
    for (size_t b = 0; b < B; b++)
        if (lut_idx[b] >= n_luts) return fail(-1, "lut_idx out of range");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    HIP_TRY(in_buf.reserve(B * BIG_CT * 8), "hipMalloc");
    HIP_TRY(out_buf.reserve(B * BIG_CT * 8), "hipMalloc");
    HIP_TRY(lutidx_buf.reserve(B * 4), "hipMalloc");
    HIP_TRY(luts_buf.reserve(n_luts * POLY_N * 8), "hipMalloc");
    HIP_TRY(hipMemcpyAsync(in_buf.ptr, in, B * BIG_CT * 8, hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipMemcpyAsync(lutidx_buf.ptr, lut_idx, B * 4, hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipMemcpyAsync(luts_buf.ptr, luts, n_luts * POLY_N * 8, hipMemcpyHostToDevice, stream), "H2D");
    int rc = pbs_batch_device(in_buf.as<uint64_t>(), lutidx_buf.as<uint32_t>(), luts_buf.as<uint64_t>(),
                              out_buf.as<uint64_t>(), B, stream, luts_low_bytes_clear(luts, n_luts * POLY_N));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, out_buf.ptr, B * BIG_CT * 8, hipMemcpyDeviceToHost, stream), "D2H");
    HIP_TRY(hipStreamSynchronize(stream), "sync");
    return 0;
}

// Rotation sharing at the raw boundary: ONE keyswitch + blind rotation per input, S sample extractions each --
// out[b][s] = what a bootstrap of (in[b] + shifts[b][s] * Delta) with LUT lut_idx[b] yields (shifts in message units,
// 0..31).  The engine does the same for rows of a level that differ only in a trivial constant (engine.cpp plan_job).
int Context::pbs_batch_shifted_host(const uint64_t *in, const uint32_t *lut_idx, const uint64_t *luts, size_t n_luts,
                                    const uint32_t *shifts, size_t S, uint64_t *out, size_t B) {
    if (!key_loaded) return fail(-3, "server key not loaded");
    if (!in || !lut_idx || !luts || !shifts || !out) return fail(-1, "null pointer");
    if (B == 0 || S == 0) return 0;
    if (B * S > (size_t)1 << 22) return fail(-1, "batch too large");
    for (size_t b = 0; b < B; b++)
        if (lut_idx[b] >= n_luts) return fail(-1, "lut_idx out of range");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    // device layout: [B rotation outputs | B body polynomials (2049-word rows) | B * S extractions]
    HIP_TRY(in_buf.reserve(B * BIG_CT * 8), "hipMalloc");
    HIP_TRY(out_buf.reserve((2 * B + B * S) * BIG_CT * 8), "hipMalloc");
    HIP_TRY(lutidx_buf.reserve(B * 4), "hipMalloc");
    HIP_TRY(luts_buf.reserve(n_luts * POLY_N * 8), "hipMalloc");
    HIP_TRY(ks_buf.reserve(B * SMALL_CT * sizeof(uint64_t)), "hipMalloc ks");
    uint64_t *d_rot = out_buf.as<uint64_t>(), *d_body = d_rot + B * BIG_CT, *d_ext = d_body + B * BIG_CT;
    std::vector<uint64_t *> ptrs(2 * B);
    std::vector<ExtractDesc> descs(B * S);
    for (size_t b = 0; b < B; b++) {
        ptrs[b] = d_rot + b * BIG_CT;
        ptrs[B + b] = d_body + b * BIG_CT;
        for (size_t k = 0; k < S; k++)
            descs[b * S + k] = ExtractDesc{ptrs[b], ptrs[B + b], d_ext + (b * S + k) * BIG_CT, 128u * (shifts[b * S + k] & 31u), 0};
    }
    DevBuf &tab = tab_buf;
    const size_t tab_bytes = ptrs.size() * sizeof(uint64_t *) + descs.size() * sizeof(ExtractDesc);
    HIP_TRY(tab.reserve(tab_bytes), "hipMalloc");
    HIP_TRY(hipMemcpyAsync(tab.ptr, ptrs.data(), ptrs.size() * sizeof(uint64_t *), hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipMemcpyAsync(tab.as<uint8_t>() + ptrs.size() * sizeof(uint64_t *), descs.data(), descs.size() * sizeof(ExtractDesc),
                           hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipMemcpyAsync(in_buf.ptr, in, B * BIG_CT * 8, hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipMemcpyAsync(lutidx_buf.ptr, lut_idx, B * 4, hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipMemcpyAsync(luts_buf.ptr, luts, n_luts * POLY_N * 8, hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipStreamSynchronize(stream), "sync");                       // the host vectors above are pageable
    if (int rc = keyswitch(in_buf.as<uint64_t>(), B, stream)) return rc;
    uint64_t *const *d_ptrs = tab.as<uint64_t *>();
    if (int rc = blind_rotate(ks_buf.as<uint64_t>(), lutidx_buf.as<uint32_t>(), luts_buf.as<uint64_t>(),
                              luts_low_bytes_clear(luts, n_luts * POLY_N), nullptr, d_ptrs, B, stream, d_ptrs + B))
        return rc;
    HIP_TRY(launch_extract_shift(reinterpret_cast<const ExtractDesc *>(tab.as<uint8_t>() + ptrs.size() * sizeof(uint64_t *)),
                                 (int)(B * S), stream), "extract launch");
    HIP_TRY(hipMemcpyAsync(out, d_ext, B * S * BIG_CT * 8, hipMemcpyDeviceToHost, stream), "D2H");
    HIP_TRY(hipStreamSynchronize(stream), "sync");
    return 0;
}

// kernel-level tests: blind rotation + sample extraction only, from given keyswitched LWEs (u64 torus, mod-switched in
// the kernel like always), in the selected arithmetic
int Context::blind_rotate_host(const uint64_t *ks, const uint32_t *lut_idx, const uint64_t *luts, size_t n_luts,
                               uint64_t *out, size_t B) {
    if (!key_loaded) return fail(-3, "server key not loaded");
    if (!ks || !lut_idx || !luts || !out) return fail(-1, "null pointer");
    if (B == 0) return 0;
    for (size_t b = 0; b < B; b++)
        if (lut_idx[b] >= n_luts) return fail(-1, "lut_idx out of range");
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    HIP_TRY(ks_buf.reserve(B * SMALL_CT * 8), "hipMalloc");
    HIP_TRY(out_buf.reserve(B * BIG_CT * 8), "hipMalloc");
    HIP_TRY(lutidx_buf.reserve(B * 4), "hipMalloc");
    HIP_TRY(luts_buf.reserve(n_luts * POLY_N * 8), "hipMalloc");
    HIP_TRY(hipMemcpyAsync(ks_buf.ptr, ks, B * SMALL_CT * 8, hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipMemcpyAsync(lutidx_buf.ptr, lut_idx, B * 4, hipMemcpyHostToDevice, stream), "H2D");
    HIP_TRY(hipMemcpyAsync(luts_buf.ptr, luts, n_luts * POLY_N * 8, hipMemcpyHostToDevice, stream), "H2D");
    if (int rc = blind_rotate(ks_buf.as<uint64_t>(), lutidx_buf.as<uint32_t>(), luts_buf.as<uint64_t>(),
                              luts_low_bytes_clear(luts, n_luts * POLY_N), out_buf.as<uint64_t>(), nullptr, B, stream))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, out_buf.ptr, B * BIG_CT * 8, hipMemcpyDeviceToHost, stream), "D2H");
    HIP_TRY(hipStreamSynchronize(stream), "sync");
    return 0;
}

int Context::ks_ms_batch_host(const uint64_t *in, uint32_t *ms_out, size_t B) {
    if (!key_loaded) return fail(-3, "server key not loaded");
    if (!in || !ms_out) return fail(-1, "null pointer");
    if (B == 0) return 0;
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    HIP_TRY(in_buf.reserve(B * BIG_CT * 8), "hipMalloc");
    HIP_TRY(ms_buf.reserve(B * SMALL_CT * 4), "hipMalloc");
    HIP_TRY(ks_buf.reserve(B * SMALL_CT * 8), "hipMalloc");
    HIP_TRY(hipMemcpyAsync(in_buf.ptr, in, B * BIG_CT * 8, hipMemcpyHostToDevice, stream), "H2D");
    if (int rc = keyswitch(in_buf.as<uint64_t>(), B, stream)) return rc;
    HIP_TRY(launch_modswitch(ks_buf.as<uint64_t>(), ms_buf.as<uint32_t>(), (int)B, stream), "modswitch launch");
    HIP_TRY(hipMemcpyAsync(ms_out, ms_buf.ptr, B * SMALL_CT * 4, hipMemcpyDeviceToHost, stream), "D2H");
    HIP_TRY(hipStreamSynchronize(stream), "sync");
    return 0;
}

}  // namespace fhs
