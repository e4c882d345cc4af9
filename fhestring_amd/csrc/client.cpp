// Client side: host-CPU mirror of MyClientKey (src/client_key.rs) -- key generation, encryption and
// decryption of FheAsciiChar / FheString under PARAM_MESSAGE_2_CARRY_2_KS_PBS.  The reference does
// this on the CPU through tfhe::integer::{gen_keys_radix, RadixClientKey}, seeded from the OS CSPRNG
// (concrete-csprng, Cargo.lock:157-165); so does this file: all secret keys, masks and noise come from
// ChaCha20 (RFC 8439 block function) keyed with 256 bits of getrandom(2) entropy, with separate
// (key, nonce) streams for secret keys, public masks and noise, so that nothing published (masks) reveals
// generator state used for anything secret.  fhs_client_create_insecure_seeded derives the ChaCha key from a
// 64-bit seed instead: reproducible keys for tests, benchmarks and multi-rank runs -- never for real data.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/fhestring_hip.h"
#include "chacha_rng.h"
#include "pbs_kernels.h"

namespace {

using namespace fhs;
using namespace fhs_rng;
constexpr double LWE_NOISE = 7.069849454709433e-6;
constexpr int PBS_BASE_LOG = 23;

}  // namespace

struct fhs_client {
    uint64_t seed = 0;            // only meaningful for insecure seeded clients (0 otherwise); kept in key files
    bool insecure = false;        // fhs_client_create_insecure_seeded: public seeds are derived from `seed` (tests)
    ChaKey key{};
    std::vector<uint64_t> lwe_sk, glwe_sk, bsk, ksk;
    std::vector<uint64_t> bsk_mb2;   // pair key of FHS_ARITH_F64_FFT_MB2, generated on first use
    std::mutex mb2_mu;
    Rng enc_mask, enc_noise;      // encryption streams: public masks and noise never share a stream
    std::atomic<uint64_t> str_calls{0};   // fhs_client_encrypt_str: every call (and every character of it) has its own streams
    std::atomic<uint64_t> cstr_calls{0};  // fhs_client_encrypt_str_compressed: the same, in a noise-stream range of its own
    // compressed server key (fhs_client_compressed_server_key), generated on first use
    ChaKey cseed{};
    std::vector<uint64_t> cbsk_bodies, cksk_bodies;
    std::mutex csk_mu;
    std::vector<uint64_t> pack_key;   // automorphism keyswitch keys of the packed result download, generated on first use
    std::mutex pack_mu;
    // public key (fhs_client_public_key): public seed of A and B = A S + E, generated on first use
    ChaKey pk_seed{};
    std::vector<uint64_t> pk_body;
    std::mutex pk_mu;
};

namespace {

// negacyclic a (*) S, S binary
void mul_binary(const uint64_t *a, const uint64_t *s, uint64_t *out) {
    std::memset(out, 0, POLY_N * 8);
    for (int j = 0; j < POLY_N; j++) {
        if (!s[j]) continue;
        for (int k = 0; k < j; k++) out[k] -= a[k + POLY_N - j];
        for (int k = j; k < POLY_N; k++) out[k] += a[k - j];
    }
}

void keygen(fhs_client *ck) {
    Rng r(ck->key, 1, DOM_SECRET);
    ck->lwe_sk.resize(LWE_N);
    ck->glwe_sk.resize(POLY_N);
    for (auto &b : ck->lwe_sk) b = r.next() >> 63;
    for (auto &b : ck->glwe_sk) b = r.next() >> 63;
    ck->bsk.assign((size_t)LWE_N * 4 * POLY_N, 0);
    ck->ksk.assign((size_t)BIG_N * KS_LEVEL * SMALL_CT, 0);
    const uint64_t qmask = ~((1ull << BSK_QUANT_BITS) - 1), qhalf = 1ull << (BSK_QUANT_BITS - 1);
    unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    // bootstrapping key: GGSW_i(lwe_sk[i]) with one level of base 2^23, on the 58-bit torus grid
    auto bsk_work = [&](unsigned tid) {
        std::vector<uint64_t> prod(POLY_N);
        for (int i = tid; i < LWE_N; i += nt) {
            Rng g(ck->key, 1000 + i, DOM_MASK), e(ck->key, 1000 + i, DOM_NOISE);
            for (int row = 0; row < 2; row++) {
                uint64_t *mask = ck->bsk.data() + (((size_t)i * 2 + row) * 2 + 0) * POLY_N;
                uint64_t *body = mask + POLY_N;
                for (int n = 0; n < POLY_N; n++) mask[n] = g.next() & qmask;
                mul_binary(mask, ck->glwe_sk.data(), prod.data());
                for (int n = 0; n < POLY_N; n++) {
                    uint64_t m;
                    if (row == 0) m = (uint64_t)0 - ((ck->lwe_sk[i] * ck->glwe_sk[n]) << (64 - PBS_BASE_LOG));
                    else m = n == 0 ? ck->lwe_sk[i] << (64 - PBS_BASE_LOG) : 0;
                    body[n] = (prod[n] + e.noise(GLWE_NOISE) + m + qhalf) & qmask;
                }
            }
        }
    };
    // keyswitching key: ksk[i][l] = LWE_small(glwe_sk[i] * 2^(64 - 3(l+1)))
    auto ksk_work = [&](unsigned tid) {
        for (int i = tid; i < BIG_N; i += nt) {
            Rng g(ck->key, 100000 + i, DOM_MASK), e(ck->key, 100000 + i, DOM_NOISE);
            for (int l = 0; l < KS_LEVEL; l++) {
                uint64_t *ct = ck->ksk.data() + ((size_t)i * KS_LEVEL + l) * SMALL_CT;
                uint64_t acc = 0;
                for (int j = 0; j < LWE_N; j++) {
                    ct[j] = g.next();
                    acc += ct[j] * ck->lwe_sk[j];
                }
                ct[LWE_N] = acc + e.noise(LWE_NOISE) + (ck->glwe_sk[i] << (64 - KS_BASE_LOG * (l + 1)));
            }
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] { bsk_work(t); ksk_work(t); });
    for (auto &x : th) x.join();
}

// Pair key of the two-bits-per-product blind rotation (fftmb_kernels.hip): for every pair (s, s') = (lwe_sk[2p],
// lwe_sk[2p+1]) three GGSWs, of s(1-s'), (1-s)s' and s s', with the bootstrapping key's own parameters (GLWE noise, one
// level of base 2^23, 58-bit grid) and their own mask / noise streams.
void keygen_mb2(fhs_client *ck) {
    ck->bsk_mb2.assign((size_t)(LWE_N / 2) * 3 * 4 * POLY_N, 0);
    const uint64_t qmask = ~((1ull << BSK_QUANT_BITS) - 1), qhalf = 1ull << (BSK_QUANT_BITS - 1);
    unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    auto work = [&](unsigned tid) {
        std::vector<uint64_t> prod(POLY_N);
        for (int g = tid; g < (LWE_N / 2) * 3; g += nt) {
            const int p = g / 3, t = g % 3;
            const uint64_t s1 = ck->lwe_sk[2 * p], s2 = ck->lwe_sk[2 * p + 1];
            const uint64_t msg = t == 0 ? s1 & (1 - s2) : t == 1 ? (1 - s1) & s2 : s1 & s2;
            Rng gm(ck->key, 2000000 + g, DOM_MASK), e(ck->key, 2000000 + g, DOM_NOISE);
            for (int row = 0; row < 2; row++) {
                uint64_t *mask = ck->bsk_mb2.data() + (((size_t)g * 2 + row) * 2 + 0) * POLY_N;
                uint64_t *body = mask + POLY_N;
                for (int n = 0; n < POLY_N; n++) mask[n] = gm.next() & qmask;
                mul_binary(mask, ck->glwe_sk.data(), prod.data());
                for (int n = 0; n < POLY_N; n++) {
                    uint64_t m;
                    if (row == 0) m = (uint64_t)0 - ((msg * ck->glwe_sk[n]) << (64 - PBS_BASE_LOG));
                    else m = n == 0 ? msg << (64 - PBS_BASE_LOG) : 0;
                    body[n] = (prod[n] + e.noise(GLWE_NOISE) + m + qhalf) & qmask;
                }
            }
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] { work(t); });
    for (auto &x : th) x.join();
}

void encrypt_block_with(const fhs_client *ck, Rng &mask, Rng &noise, uint64_t m, uint64_t *ct) {
    mask.fill(ct, BIG_N);
    uint64_t acc = 0;
    const uint64_t *sk = ck->glwe_sk.data();
    for (int j = 0; j < BIG_N; j++) acc += ct[j] & ((uint64_t)0 - sk[j]);   // binary key
    ct[BIG_N] = acc + noise.noise(GLWE_NOISE) + (m << DELTA_LOG);
}
void encrypt_block(fhs_client *ck, uint64_t m, uint64_t *ct) { encrypt_block_with(ck, ck->enc_mask, ck->enc_noise, m, ct); }
// host threads for the per-character work of one string (encryption: 16 KB of ChaCha20 keystream and a 2048-term masked
// sum per block; decryption: a 2048-term product): config 5 hands over 2 x 4097 characters = 537 MB of ciphertext, which
// one thread needs ~0.16 s for -- as long as the GPU needs for the whole op (VERDICT r4 "missing 5")
unsigned string_threads(size_t n_chars) {
    unsigned hw = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    if (const char *e = std::getenv("FHS_CLIENT_THREADS")) hw = (unsigned)std::max(1, std::atoi(e));   // tests: 1 = sequential
    return (unsigned)std::max<size_t>(1, std::min<size_t>(hw, n_chars / 32));
}
template <class F>
void for_each_char(size_t n, F &&f) {
    const unsigned nt = string_threads(n);
    if (nt <= 1) {
        for (size_t i = 0; i < n; i++) f(i);
        return;
    }
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t i0 = next.fetch_add(16);
            if (i0 >= n) return;
            for (size_t i = i0; i < std::min(n, i0 + 16); i++) f(i);
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &x : th) x.join();
}
constexpr uint64_t STR_STREAM_BASE = 1ull << 62;   // stream ids of string encryptions: base + (call << 24) + character
constexpr size_t STR_MAX_CHARS = (size_t)1 << 24;
uint64_t decrypt_block(const fhs_client *ck, const uint64_t *ct) {
    uint64_t acc = 0;
    for (int j = 0; j < BIG_N; j++) acc += ct[j] * ck->glwe_sk[j];
    const uint64_t ph = ct[BIG_N] - acc;
    return ((ph + (1ull << (DELTA_LOG - 1))) >> DELTA_LOG) & 31;
}

}  // namespace

extern "C" {

static int client_create_with_key(const ChaKey &k, uint64_t seed, fhs_client **out) {
    fhs_client *ck = new (std::nothrow) fhs_client();
    if (!ck) return FHS_ERR_STATE;
    ck->seed = seed;
    ck->key = k;
    ck->enc_mask = Rng(k, 7, DOM_MASK);
    ck->enc_noise = Rng(k, 7, DOM_NOISE);
    keygen(ck);
    *out = ck;
    return FHS_OK;
}
// diagnostic: one ChaCha20 block of the generator (known-answer test against RFC 8439 section 2.3.2)
void fhs_chacha20_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]) {
    ChaKey k;
    for (int i = 0; i < 8; i++) k.w[i] = key[i];
    Rng r(k, 0, 0);
    r.st[12] = counter; r.st[13] = nonce[0]; r.st[14] = nonce[1]; r.st[15] = nonce[2];
    r.refill();
    for (int i = 0; i < 16; i++) out[i] = r.buf[i];
}
// diagnostic: n 64-bit draws of the generator from that state (the keystream in order, whichever block routine made it)
void fhs_chacha20_stream(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint64_t *out, size_t n) {
    ChaKey k;
    for (int i = 0; i < 8; i++) k.w[i] = key[i];
    Rng r(k, 0, 0);
    r.st[12] = counter; r.st[13] = nonce[0]; r.st[14] = nonce[1]; r.st[15] = nonce[2];
    for (size_t i = 0; i < n; i++) out[i] = r.next();
}
int fhs_client_create(fhs_client **out) {   // MyClientKey::from_params (client_key.rs:30-35): OS-seeded CSPRNG
    if (!out) return FHS_ERR_ARG;
    ChaKey k;
    if (!os_entropy(&k, sizeof(k))) return FHS_ERR_STATE;
    return client_create_with_key(k, 0, out);
}
int fhs_client_create_insecure_seeded(uint64_t seed, fhs_client **out) {   // tests / benchmarks / identical keys on every rank
    if (!out) return FHS_ERR_ARG;
    const int rc = client_create_with_key(key_from_seed(seed), seed, out);
    if (rc == FHS_OK) (*out)->insecure = true;
    return rc;
}
void fhs_client_destroy(fhs_client *ck) { delete ck; }
const uint64_t *fhs_client_bsk(const fhs_client *ck) { return ck ? ck->bsk.data() : nullptr; }
const uint64_t *fhs_client_ksk(const fhs_client *ck) { return ck ? ck->ksk.data() : nullptr; }
const uint64_t *fhs_client_bsk_mb2(fhs_client *ck) {
    if (!ck) return nullptr;
    std::lock_guard<std::mutex> lk(ck->mb2_mu);
    if (ck->bsk_mb2.empty()) keygen_mb2(ck);
    return ck->bsk_mb2.data();
}

int fhs_client_encrypt_char(fhs_client *ck, uint8_t v, uint64_t *blocks) {   // FheAsciiChar::encrypt (fheasciichar.rs:27-29)
    if (!ck || !blocks) return FHS_ERR_ARG;
    for (int b = 0; b < 4; b++) encrypt_block(ck, (v >> (2 * b)) & 3, blocks + (size_t)b * BIG_CT);
    return FHS_OK;
}
int fhs_client_decrypt_char(const fhs_client *ck, const uint64_t *blocks, uint8_t *out) {   // decrypt::<u8> (:31-33)
    if (!ck || !blocks || !out) return FHS_ERR_ARG;
    unsigned v = 0;
    for (int b = 0; b < 4; b++) v += (unsigned)(decrypt_block(ck, blocks + (size_t)b * BIG_CT) & 15) << (2 * b);
    *out = (uint8_t)(v & 255);
    return FHS_OK;
}
int fhs_client_encrypt_str(fhs_client *ck, const char *s, size_t len, size_t padding, uint64_t *out) {   // encrypt (:45-65)
    if (!ck || (len && !s) || !out) return FHS_ERR_ARG;
    for (size_t i = 0; i < len; i++)
        if ((unsigned char)s[i] >= 128 || s[i] == 0) return FHS_ERR_ARG;   // the reference asserts ASCII, no NUL (:52-55)
    const size_t n = len + padding;
    if (n > STR_MAX_CHARS) return FHS_ERR_LIMIT;
    // Every character draws from its own (mask, noise) stream pair, keyed by the call number and its index: the result
    // does not depend on how many host threads share the work, masks and noise never share a stream, and no two
    // characters of any two calls share one.  (fhs_client_encrypt_char keeps the client's sequential streams.)
    const uint64_t call = ck->str_calls.fetch_add(1);
    for_each_char(n, [&](size_t i) {
        const uint64_t sid = STR_STREAM_BASE + (call << 24) + i;
        Rng mask(ck->key, sid, DOM_MASK), noise(ck->key, sid, DOM_NOISE);
        const uint8_t v = i < len ? (uint8_t)s[i] : 0;
        for (int b = 0; b < 4; b++)
            encrypt_block_with(ck, mask, noise, (v >> (2 * b)) & 3, out + i * FHS_CHAR_WORDS + (size_t)b * BIG_CT);
    });
    return FHS_OK;
}
int fhs_client_decrypt_str(const fhs_client *ck, const uint64_t *chars, size_t n, char *out, size_t *out_len) {   // decrypt (:89-106)
    if (!ck || (n && !chars) || !out || !out_len) return FHS_ERR_ARG;
    std::vector<uint8_t> vals(n);
    for_each_char(n, [&](size_t i) { fhs_client_decrypt_char(ck, chars + i * FHS_CHAR_WORDS, &vals[i]); });
    size_t k = 0;
    for (size_t i = 0; i < n; i++) {
        if (vals[i] == 0) break;   // truncate at the first NUL (:91-96)
        out[k++] = (char)vals[i];
    }
    *out_len = k;
    return FHS_OK;
}
namespace {
struct KeyFileHeader {
    char magic[8];
    uint64_t kind, lwe_n, poly_n, ks_levels, ks_base_log, pbs_base_log, bsk_quant_bits;
};
static_assert(sizeof(KeyFileHeader) == 64, "header is 64 bytes");
KeyFileHeader make_header(uint64_t kind) {
    KeyFileHeader h{};
    std::memcpy(h.magic, "FHSKEY01", 8);
    h.kind = kind; h.lwe_n = LWE_N; h.poly_n = POLY_N; h.ks_levels = KS_LEVEL; h.ks_base_log = KS_BASE_LOG;
    h.pbs_base_log = PBS_BASE_LOG; h.bsk_quant_bits = BSK_QUANT_BITS;
    return h;
}
bool header_ok(const KeyFileHeader &h) {
    const KeyFileHeader w = make_header(h.kind);
    return std::memcmp(&h, &w, sizeof(h)) == 0 && h.kind >= 1 && h.kind <= 6;
}
bool write_all(FILE *f, const void *p, size_t n) { return std::fwrite(p, 1, n, f) == n; }
bool read_all(FILE *f, void *p, size_t n) { return std::fread(p, 1, n, f) == n; }
}  // namespace

int fhs_client_save(const fhs_client *ck, const char *path, int server_key_only) {
    if (!ck || !path) return FHS_ERR_ARG;
    FILE *f = std::fopen(path, "wb");
    if (!f) return FHS_ERR_STATE;
    const KeyFileHeader h = make_header(server_key_only ? 2 : 1);
    bool ok = write_all(f, &h, sizeof(h));
    if (!server_key_only) {
        ok = ok && write_all(f, &ck->seed, 8) && write_all(f, ck->lwe_sk.data(), ck->lwe_sk.size() * 8) &&
             write_all(f, ck->glwe_sk.data(), ck->glwe_sk.size() * 8);
    }
    ok = ok && write_all(f, ck->bsk.data(), ck->bsk.size() * 8) && write_all(f, ck->ksk.data(), ck->ksk.size() * 8);
    ok = (std::fclose(f) == 0) && ok;
    return ok ? FHS_OK : FHS_ERR_STATE;
}

// kind 3: the pair key of the two-key-bits-per-product arithmetics alone (it accompanies a kind 1 / kind 2 file)
int fhs_client_save_multibit_key(fhs_client *ck, const char *path) {
    if (!ck || !path) return FHS_ERR_ARG;
    const uint64_t *mb = fhs_client_bsk_mb2(ck);
    FILE *f = std::fopen(path, "wb");
    if (!f) return FHS_ERR_STATE;
    const KeyFileHeader h = make_header(3);
    bool ok = write_all(f, &h, sizeof(h)) && write_all(f, mb, FHS_BSK_MB2_WORDS * 8);
    ok = (std::fclose(f) == 0) && ok;
    return ok ? FHS_OK : FHS_ERR_STATE;
}
int fhs_read_multibit_key_file(const char *path, std::vector<uint64_t> &mb) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return FHS_ERR_STATE;
    KeyFileHeader h;
    bool ok = read_all(f, &h, sizeof(h)) && header_ok(h) && h.kind == 3;
    if (ok) {
        mb.resize(FHS_BSK_MB2_WORDS);
        ok = read_all(f, mb.data(), mb.size() * 8) && std::fgetc(f) == EOF;
    }
    std::fclose(f);
    return ok ? FHS_OK : FHS_ERR_STATE;
}

int fhs_client_load(const char *path, fhs_client **out) {
    if (!path || !out) return FHS_ERR_ARG;
    FILE *f = std::fopen(path, "rb");
    if (!f) return FHS_ERR_STATE;
    KeyFileHeader h;
    fhs_client *ck = new (std::nothrow) fhs_client();
    bool ok = ck && read_all(f, &h, sizeof(h)) && header_ok(h) && h.kind == 1;
    if (ok) {
        ck->lwe_sk.resize(LWE_N); ck->glwe_sk.resize(POLY_N);
        ck->bsk.resize((size_t)LWE_N * 4 * POLY_N); ck->ksk.resize((size_t)BIG_N * KS_LEVEL * SMALL_CT);
        ok = read_all(f, &ck->seed, 8) && read_all(f, ck->lwe_sk.data(), LWE_N * 8) &&
             read_all(f, ck->glwe_sk.data(), POLY_N * 8) && read_all(f, ck->bsk.data(), ck->bsk.size() * 8) &&
             read_all(f, ck->ksk.data(), ck->ksk.size() * 8);
        // a loaded client never replays an encryption stream: fresh OS entropy for masks and noise
        ok = ok && os_entropy(&ck->key, sizeof(ck->key));
        ck->enc_mask = Rng(ck->key, 7, DOM_MASK);
        ck->enc_noise = Rng(ck->key, 7, DOM_NOISE);
    }
    std::fclose(f);
    if (!ok) { delete ck; return FHS_ERR_STATE; }
    *out = ck;
    return FHS_OK;
}

// reads only the server-key part of a key file (used by fhs_load_server_key_file in capi_core.cpp)
int fhs_read_server_key_file(const char *path, std::vector<uint64_t> &bsk, std::vector<uint64_t> &ksk) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return FHS_ERR_STATE;
    KeyFileHeader h;
    bool ok = read_all(f, &h, sizeof(h)) && header_ok(h) && (h.kind == 1 || h.kind == 2);
    if (ok && h.kind == 1) ok = std::fseek(f, 8 + (LWE_N + POLY_N) * 8, SEEK_CUR) == 0;
    if (ok) {
        bsk.resize((size_t)LWE_N * 4 * POLY_N); ksk.resize((size_t)BIG_N * KS_LEVEL * SMALL_CT);
        ok = read_all(f, bsk.data(), bsk.size() * 8) && read_all(f, ksk.data(), ksk.size() * 8);
    }
    std::fclose(f);
    return ok ? FHS_OK : FHS_ERR_STATE;
}

int fhs_client_secret_keys(const fhs_client *ck, uint64_t *lwe_sk, uint64_t *glwe_sk) {
    if (!ck || !lwe_sk || !glwe_sk) return FHS_ERR_ARG;
    std::memcpy(lwe_sk, ck->lwe_sk.data(), LWE_N * 8);
    std::memcpy(glwe_sk, ck->glwe_sk.data(), POLY_N * 8);
    return FHS_OK;
}

}  // extern "C"

// ---- compressed (seeded) ciphertexts and server keys: the convention of include/fhestring_hip.h -------------------
namespace {

ChaKey seed_key(const uint32_t seed[8]) {
    ChaKey k;
    for (int i = 0; i < 8; i++) k.w[i] = seed[i];
    return k;
}
// Public seed of a compressed object: 32 bytes of OS entropy.  An insecure seeded client derives it from its 64-bit
// seed, a tag per kind of object and the call number instead (reproducible tests) -- never from its ChaCha key.
bool public_seed(const fhs_client *ck, uint64_t tag, uint64_t call, ChaKey &out) {
    if (!ck->insecure) return os_entropy(&out, sizeof(out));
    out = key_from_seed(ck->seed ^ tag);
    out.w[6] ^= (uint32_t)call;
    out.w[7] ^= (uint32_t)(call >> 32);
    return true;
}
constexpr uint64_t SEED_TAG_STR = 0x5345454453545231ull, SEED_TAG_KEY = 0x534545444b455931ull;
// Secret noise streams (DOM_NOISE) of compressed objects, disjoint from every other range of the client:
//   7 (encrypt_char), 1000 + i (BSK), 100000 + i (KSK), 2000000 + g (pair key), STR_STREAM_BASE + (call << 24) + i
//   (classic strings, [2^62, 2^63)).  Compressed strings: CSTR_STREAM_BASE + (call << 24) + character, [2^63, 2^63 + 2^62)
//   for call < 2^38; the compressed server key: 4000000 + i (BSK, key bit i), 5000000 + i (KSK, row i).
constexpr uint64_t CSTR_STREAM_BASE = 1ull << 63;
constexpr uint64_t CBSK_NOISE_BASE = 4000000, CKSK_NOISE_BASE = 5000000;

// sum_j draw_j * s_j over n draws of `mask`, s binary; the draws are streamed through a small buffer, never stored whole
uint64_t streamed_dot(Rng &mask, const uint64_t *s, int n) {
    uint64_t tmp[64], acc = 0;
    for (int j = 0; j < n; j += 64) {
        const int k = std::min(64, n - j);
        mask.fill(tmp, (size_t)k);
        for (int q = 0; q < k; q++) acc += tmp[q] & ((uint64_t)0 - s[j + q]);
    }
    return acc;
}

void keygen_compressed(fhs_client *ck) {
    ck->cbsk_bodies.assign(FHS_CBSK_BODY_WORDS, 0);
    ck->cksk_bodies.assign(FHS_CKSK_BODY_WORDS, 0);
    const uint64_t qmask = ~((1ull << BSK_QUANT_BITS) - 1), qhalf = 1ull << (BSK_QUANT_BITS - 1);
    const ChaKey seed = ck->cseed;
    // BSK: the rows of keygen's GGSW_i(lwe_sk[i]) with seeded masks
    for_each_char(LWE_N, [&](size_t i) {
        std::vector<uint64_t> mask(POLY_N), prod(POLY_N);
        Rng e(ck->key, CBSK_NOISE_BASE + i, DOM_NOISE);
        for (int row = 0; row < 2; row++) {
            Rng g(seed, 2 * i + row, FHS_DOM_SEEDED_BSK);
            for (int n = 0; n < POLY_N; n++) mask[n] = g.next() & qmask;
            mul_binary(mask.data(), ck->glwe_sk.data(), prod.data());
            uint64_t *body = ck->cbsk_bodies.data() + (i * 2 + row) * POLY_N;
            for (int n = 0; n < POLY_N; n++) {
                uint64_t m;
                if (row == 0) m = (uint64_t)0 - ((ck->lwe_sk[i] * ck->glwe_sk[n]) << (64 - PBS_BASE_LOG));
                else m = n == 0 ? ck->lwe_sk[i] << (64 - PBS_BASE_LOG) : 0;
                body[n] = (prod[n] + e.noise(GLWE_NOISE) + m + qhalf) & qmask;
            }
        }
    });
    // KSK: ksk[i][l] = LWE_small(glwe_sk[i] * 2^(64 - 3(l+1))) with seeded masks
    for_each_char(BIG_N, [&](size_t i) {
        Rng e(ck->key, CKSK_NOISE_BASE + i, DOM_NOISE);
        for (int l = 0; l < KS_LEVEL; l++) {
            Rng g(seed, (uint64_t)KS_LEVEL * i + l, FHS_DOM_SEEDED_KSK);
            const uint64_t acc = streamed_dot(g, ck->lwe_sk.data(), LWE_N);
            ck->cksk_bodies[i * KS_LEVEL + l] =
                acc + e.noise(LWE_NOISE) + (ck->glwe_sk[i] << (64 - KS_BASE_LOG * (l + 1)));
        }
    });
}
bool compressed_server_key(fhs_client *ck) {
    std::lock_guard<std::mutex> lk(ck->csk_mu);
    if (!ck->cbsk_bodies.empty()) return true;
    if (!public_seed(ck, SEED_TAG_KEY, 0, ck->cseed)) return false;
    keygen_compressed(ck);
    return true;
}

}  // namespace

extern "C" {

int fhs_client_encrypt_str_compressed(fhs_client *ck, const char *s, size_t len, size_t padding, uint32_t seed_out[8],
                                      uint64_t *bodies) {
    if (!ck || (len && !s) || !seed_out || !bodies) return FHS_ERR_ARG;
    for (size_t i = 0; i < len; i++)
        if ((unsigned char)s[i] >= 128 || s[i] == 0) return FHS_ERR_ARG;
    const size_t n = len + padding;
    if (n > STR_MAX_CHARS) return FHS_ERR_LIMIT;
    const uint64_t call = ck->cstr_calls.fetch_add(1);
    ChaKey seed;
    if (!public_seed(ck, SEED_TAG_STR, call, seed)) return FHS_ERR_STATE;
    for_each_char(n, [&](size_t i) {
        Rng noise(ck->key, CSTR_STREAM_BASE + (call << 24) + i, DOM_NOISE);
        const uint8_t v = i < len ? (uint8_t)s[i] : 0;
        for (int b = 0; b < 4; b++) {
            Rng mask(seed, 4 * i + b, FHS_DOM_SEEDED_STR);
            const uint64_t acc = streamed_dot(mask, ck->glwe_sk.data(), BIG_N);
            bodies[4 * i + b] = acc + noise.noise(GLWE_NOISE) + ((uint64_t)((v >> (2 * b)) & 3) << DELTA_LOG);
        }
    });
    for (int i = 0; i < 8; i++) seed_out[i] = seed.w[i];
    return FHS_OK;
}

int fhs_expand_compressed_str(const uint32_t seed[8], const uint64_t *bodies, size_t n, size_t first_char, uint64_t *out) {
    if (!seed || (n && (!bodies || !out))) return FHS_ERR_ARG;
    const ChaKey k = seed_key(seed);
    for_each_char(n, [&](size_t i) {
        for (int b = 0; b < 4; b++) {
            uint64_t *ct = out + i * FHS_CHAR_WORDS + (size_t)b * BIG_CT;
            Rng mask(k, 4 * (first_char + i) + b, FHS_DOM_SEEDED_STR);
            mask.fill(ct, BIG_N);
            ct[BIG_N] = bodies[4 * i + b];
        }
    });
    return FHS_OK;
}

int fhs_client_compressed_server_key(fhs_client *ck, uint32_t seed_out[8], uint64_t *bsk_bodies, uint64_t *ksk_bodies) {
    if (!ck || !seed_out || !bsk_bodies || !ksk_bodies) return FHS_ERR_ARG;
    if (!compressed_server_key(ck)) return FHS_ERR_STATE;
    for (int i = 0; i < 8; i++) seed_out[i] = ck->cseed.w[i];
    std::memcpy(bsk_bodies, ck->cbsk_bodies.data(), FHS_CBSK_BODY_WORDS * 8);
    std::memcpy(ksk_bodies, ck->cksk_bodies.data(), FHS_CKSK_BODY_WORDS * 8);
    return FHS_OK;
}

int fhs_client_save_compressed_server_key(fhs_client *ck, const char *path) {
    if (!ck || !path) return FHS_ERR_ARG;
    if (!compressed_server_key(ck)) return FHS_ERR_STATE;
    FILE *f = std::fopen(path, "wb");
    if (!f) return FHS_ERR_STATE;
    const KeyFileHeader h = make_header(4);
    bool ok = write_all(f, &h, sizeof(h)) && write_all(f, ck->cseed.w, 32) &&
              write_all(f, ck->cbsk_bodies.data(), FHS_CBSK_BODY_WORDS * 8) &&
              write_all(f, ck->cksk_bodies.data(), FHS_CKSK_BODY_WORDS * 8);
    ok = (std::fclose(f) == 0) && ok;
    return ok ? FHS_OK : FHS_ERR_STATE;
}
// reads a kind 4 file (used by fhs_load_compressed_server_key_file in capi_core.cpp)
int fhs_read_compressed_server_key_file(const char *path, uint32_t seed[8], std::vector<uint64_t> &bsk_bodies,
                                        std::vector<uint64_t> &ksk_bodies) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return FHS_ERR_STATE;
    KeyFileHeader h;
    bool ok = read_all(f, &h, sizeof(h)) && header_ok(h) && h.kind == 4;
    if (ok) {
        bsk_bodies.resize(FHS_CBSK_BODY_WORDS);
        ksk_bodies.resize(FHS_CKSK_BODY_WORDS);
        ok = read_all(f, seed, 32) && read_all(f, bsk_bodies.data(), bsk_bodies.size() * 8) &&
             read_all(f, ksk_bodies.data(), ksk_bodies.size() * 8) && std::fgetc(f) == EOF;
    }
    std::fclose(f);
    return ok ? FHS_OK : FHS_ERR_STATE;
}

int fhs_expand_compressed_server_key(const uint32_t seed[8], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies,
                                     uint64_t *bsk, uint64_t *ksk) {
    if (!seed || !bsk_bodies || !ksk_bodies || !bsk || !ksk) return FHS_ERR_ARG;
    const ChaKey k = seed_key(seed);
    const uint64_t qmask = ~((1ull << BSK_QUANT_BITS) - 1);
    for_each_char((size_t)LWE_N * 2, [&](size_t p) {          // GGSW row p = 2i + r
        uint64_t *mask = bsk + p * 2 * POLY_N;
        Rng g(k, p, FHS_DOM_SEEDED_BSK);
        for (int n = 0; n < POLY_N; n++) mask[n] = g.next() & qmask;
        std::memcpy(mask + POLY_N, bsk_bodies + p * POLY_N, POLY_N * 8);
    });
    for_each_char((size_t)BIG_N * KS_LEVEL, [&](size_t r) {   // row r = 5i + l
        uint64_t *ct = ksk + r * SMALL_CT;
        Rng g(k, r, FHS_DOM_SEEDED_KSK);
        g.fill(ct, LWE_N);
        ct[LWE_N] = ksk_bodies[r];
    });
    return FHS_OK;
}

}  // extern "C"

// ---- packed result download (pack_host.cpp, pack_kernels.hip): key material and decryption ----------------------------
namespace {

// Automorphism keyswitch keys of the ring packing: for tree level lv = 1..11 (g = 2^lv + 1) and digit level l,
// K[lv-1][l] = (mask, body) is a GLWE encryption under S of S(X^g) * 2^(64 - PACK_BASE_LOG (l + 1)), with the bootstrapping
// key's noise and 58-bit grid.  Streams 6000000 + 3 (lv - 1) + l (DOM_MASK / DOM_NOISE), a range of their own.
constexpr uint64_t PACK_STREAM_BASE = 6000000;
void keygen_packing(fhs_client *ck) {
    ck->pack_key.assign(FHS_PACK_KEY_WORDS, 0);
    const uint64_t qmask = ~((1ull << BSK_QUANT_BITS) - 1), qhalf = 1ull << (BSK_QUANT_BITS - 1);
    std::vector<std::thread> th;
    for (int lv = 1; lv <= FHS_PACK_TREE_LEVELS; lv++) {
        th.emplace_back([=] {
            const uint32_t g = (1u << lv) + 1;
            std::vector<uint64_t> sg(POLY_N), prod(POLY_N);
            for (uint32_t i = 0; i < (uint32_t)POLY_N; i++) {          // S(X^g): coefficient i goes to i g mod 2N
                const uint32_t r = (i * g) & (2 * POLY_N - 1);
                sg[r & (POLY_N - 1)] = r >= (uint32_t)POLY_N ? (uint64_t)0 - ck->glwe_sk[i] : ck->glwe_sk[i];
            }
            for (int l = 0; l < FHS_PACK_LEVELS; l++) {
                const uint64_t sid = PACK_STREAM_BASE + (uint64_t)FHS_PACK_LEVELS * (lv - 1) + l;
                Rng gm(ck->key, sid, DOM_MASK), e(ck->key, sid, DOM_NOISE);
                uint64_t *mask = ck->pack_key.data() + (((size_t)(lv - 1) * FHS_PACK_LEVELS + l) * 2) * POLY_N;
                uint64_t *body = mask + POLY_N;
                for (int n = 0; n < POLY_N; n++) mask[n] = gm.next() & qmask;
                mul_binary(mask, ck->glwe_sk.data(), prod.data());
                for (int n = 0; n < POLY_N; n++)
                    body[n] = (prod[n] + e.noise(GLWE_NOISE) + (sg[n] << (64 - FHS_PACK_BASE_LOG * (l + 1))) + qhalf) & qmask;
            }
        });
    }
    for (auto &x : th) x.join();
}

// phases of one packed group: ph[j] = (body16[j] << 48) - ((mask16 << 48) (*) S)[j], j < count
void packed_phases(const fhs_client *ck, const uint16_t *mask16, const uint16_t *body16, size_t count, uint64_t *ph) {
    std::vector<uint64_t> a(POLY_N), prod(POLY_N);
    for (int i = 0; i < POLY_N; i++) a[i] = (uint64_t)mask16[i] << 48;
    mul_binary(a.data(), ck->glwe_sk.data(), prod.data());
    for (size_t j = 0; j < count; j++) ph[j] = ((uint64_t)body16[j] << 48) - prod[j];
}

}  // namespace

extern "C" {

const uint64_t *fhs_client_packing_key(fhs_client *ck) {
    if (!ck) return nullptr;
    std::lock_guard<std::mutex> lk(ck->pack_mu);
    if (ck->pack_key.empty()) keygen_packing(ck);
    return ck->pack_key.data();
}

// kind 5: the packing key alone (it accompanies a kind 1 / 2 / 4 file, like kind 3)
int fhs_client_save_packing_key(fhs_client *ck, const char *path) {
    if (!ck || !path) return FHS_ERR_ARG;
    const uint64_t *k = fhs_client_packing_key(ck);
    FILE *f = std::fopen(path, "wb");
    if (!f) return FHS_ERR_STATE;
    KeyFileHeader h = make_header(5);
    bool ok = write_all(f, &h, sizeof(h)) && write_all(f, k, FHS_PACK_KEY_WORDS * 8);
    ok = (std::fclose(f) == 0) && ok;
    return ok ? FHS_OK : FHS_ERR_STATE;
}

int fhs_client_encrypt_blocks(fhs_client *ck, const uint8_t *values, size_t n, uint64_t *blocks) {
    if (!ck || (n && (!values || !blocks))) return FHS_ERR_ARG;
    for (size_t i = 0; i < n; i++) encrypt_block(ck, values[i] & 31, blocks + i * BIG_CT);
    return FHS_OK;
}

int fhs_client_decrypt_packed_blocks(const fhs_client *ck, const void *mask16_, const void *body16_, size_t n_blocks,
                                     uint8_t *out) {
    const uint16_t *mask16 = static_cast<const uint16_t *>(mask16_), *body16 = static_cast<const uint16_t *>(body16_);
    if (!ck || (n_blocks && (!mask16 || !body16 || !out))) return FHS_ERR_ARG;
    std::vector<uint64_t> ph(FHS_PACK_GROUP);
    for (size_t g = 0; g * FHS_PACK_GROUP < n_blocks; g++) {
        const size_t count = std::min<size_t>(FHS_PACK_GROUP, n_blocks - g * FHS_PACK_GROUP);
        packed_phases(ck, mask16 + g * POLY_N, body16 + g * FHS_PACK_GROUP, count, ph.data());
        for (size_t j = 0; j < count; j++)
            out[g * FHS_PACK_GROUP + j] = (uint8_t)(((ph[j] + (1ull << (DELTA_LOG - 1))) >> DELTA_LOG) & 31);
    }
    return FHS_OK;
}

int fhs_client_decrypt_packed_str(const fhs_client *ck, const void *mask16, const void *body16, size_t n_chars,
                                  char *out, size_t *out_len) {
    if (!ck || !out || !out_len || (n_chars && (!mask16 || !body16))) return FHS_ERR_ARG;
    std::vector<uint8_t> blk(4 * n_chars);
    if (int rc = fhs_client_decrypt_packed_blocks(ck, mask16, body16, 4 * n_chars, blk.data())) return rc;
    size_t k = 0;
    for (size_t i = 0; i < n_chars; i++) {
        unsigned v = 0;
        for (int b = 0; b < 4; b++) v += (unsigned)(blk[4 * i + b] & 15) << (2 * b);   // as fhs_client_decrypt_char
        if ((v & 255) == 0) break;   // truncate at the first NUL
        out[k++] = (char)(v & 255);
    }
    *out_len = k;
    return FHS_OK;
}

}  // extern "C"

// reads a kind 5 file (used by fhs_load_packing_key_file in capi_ops.cpp)
int fhs_read_packing_key_file(const char *path, std::vector<uint64_t> &key) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return FHS_ERR_STATE;
    KeyFileHeader h;
    bool ok = read_all(f, &h, sizeof(h)) && header_ok(h) && h.kind == 5;
    if (ok) {
        key.resize(FHS_PACK_KEY_WORDS);
        ok = read_all(f, key.data(), key.size() * 8) && std::fgetc(f) == EOF;
    }
    std::fclose(f);
    return ok ? FHS_OK : FHS_ERR_STATE;
}

// ---- public key (pk_host.cpp, pk_kernels.hip): the client's side ---------------------------------------------------------
namespace {

// B = A S + E in Z_2^64[X]/(X^2048+1): A = 2048 draws of the public seed's stream (domain FHS_DOM_PUBLIC_KEY, stream 0),
// E from the secret noise stream PK_NOISE_STREAM, a range of its own beside those listed above.
constexpr uint64_t SEED_TAG_PK = 0x53454544504b3031ull, PK_NOISE_STREAM = 7000000;
bool public_key(fhs_client *ck) {
    std::lock_guard<std::mutex> lk(ck->pk_mu);
    if (!ck->pk_body.empty()) return true;
    if (!public_seed(ck, SEED_TAG_PK, 0, ck->pk_seed)) return false;
    std::vector<uint64_t> a(POLY_N), body(POLY_N);
    Rng g(ck->pk_seed, 0, FHS_DOM_PUBLIC_KEY), e(ck->key, PK_NOISE_STREAM, DOM_NOISE);
    g.fill(a.data(), POLY_N);
    mul_binary(a.data(), ck->glwe_sk.data(), body.data());
    for (int n = 0; n < POLY_N; n++) body[n] += e.noise(GLWE_NOISE);
    ck->pk_body.swap(body);
    return true;
}

}  // namespace

extern "C" {

int fhs_client_public_key(fhs_client *ck, uint32_t seed_out[8], uint64_t *body_out) {
    if (!ck || !seed_out || !body_out) return FHS_ERR_ARG;
    if (!public_key(ck)) return FHS_ERR_STATE;
    for (int i = 0; i < 8; i++) seed_out[i] = ck->pk_seed.w[i];
    std::memcpy(body_out, ck->pk_body.data(), POLY_N * 8);
    return FHS_OK;
}

// kind 6: header, seed (32 B), B (2048 words).  No secret in it.
int fhs_client_save_public_key(fhs_client *ck, const char *path) {
    if (!ck || !path) return FHS_ERR_ARG;
    if (!public_key(ck)) return FHS_ERR_STATE;
    FILE *f = std::fopen(path, "wb");
    if (!f) return FHS_ERR_STATE;
    const KeyFileHeader h = make_header(6);
    bool ok = write_all(f, &h, sizeof(h)) && write_all(f, ck->pk_seed.w, 32) && write_all(f, ck->pk_body.data(), POLY_N * 8);
    ok = (std::fclose(f) == 0) && ok;
    return ok ? FHS_OK : FHS_ERR_STATE;
}

}  // extern "C"

// reads a kind 6 file (used by fhs_public_key_load in pk_host.cpp)
int fhs_read_public_key_file(const char *path, uint32_t seed[8], std::vector<uint64_t> &body) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return FHS_ERR_STATE;
    KeyFileHeader h;
    bool ok = read_all(f, &h, sizeof(h)) && header_ok(h) && h.kind == 6;
    if (ok) {
        body.resize(POLY_N);
        ok = read_all(f, seed, 32) && read_all(f, body.data(), body.size() * 8) && std::fgetc(f) == EOF;
    }
    std::fclose(f);
    return ok ? FHS_OK : FHS_ERR_STATE;
}
