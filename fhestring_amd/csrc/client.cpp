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
#include <cstdlib>
#include <cstring>
#include <new>
#include <mutex>
#include <vector>

#include "../../include/fhestring_hip.h"
#include "chacha_rng.h"
#include "host_ntt.h"
#include "host_parallel.h"
#include "keyfile.h"
#include "pbs_kernels.h"

namespace {

using namespace fhs;
using namespace fhs_rng;
constexpr double LWE_NOISE = 7.069849454709433e-6;

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
    std::atomic<uint64_t> rekey_calls{0};   // re-key keys made INTO this client (fhs_client_rekey_key): one ChaCha key each
    std::atomic<uint64_t> select_calls{0};  // select queries made by this client (fhs_client_select_query): one ChaCha key each
    std::atomic<uint64_t> sselect_calls{0}; // seeded select queries (fhs_client_select_query_seeded): a seed and noise streams each
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

// The 58-bit torus grid of the bootstrapping and packing keys: masks are truncated to it, bodies rounded (round_to_grid).
constexpr uint64_t GRID_MASK = ~((1ull << BSK_QUANT_BITS) - 1);

// The two body rows of GGSW(msg) from its two mask rows, msg a key bit or a product of key bits: one level of base 2^23,
// body[r] = mask[r] (*) S + noise + the row's message, -msg S 2^(64-23) for row 0 and msg 2^(64-23) for row 1, on the
// grid.  2 x 2048 draws of `noise`, row 0 first.
void ggsw_bodies(const fhs_client *ck, uint64_t msg, Rng &noise, const uint64_t *const mask[2], uint64_t *const body[2]) {
    std::vector<uint64_t> prod(POLY_N);
    for (int r = 0; r < 2; r++) {
        mul_binary(mask[r], ck->glwe_sk.data(), prod.data());
        for (int n = 0; n < POLY_N; n++) {
            uint64_t m;
            if (r == 0) m = (uint64_t)0 - ((msg * ck->glwe_sk[n]) << (64 - PBS_BASE_LOG));
            else m = n == 0 ? msg << (64 - PBS_BASE_LOG) : 0;
            body[r][n] = round_to_grid(prod[n] + noise.noise(GLWE_NOISE) + m, BSK_QUANT_BITS);
        }
    }
}
// GGSW(msg) in the layout of the bootstrapping keys, [row][mask, body][2048]: 2 x 2048 draws of `mask`, row 0 first
void ggsw_encrypt(const fhs_client *ck, uint64_t msg, Rng &mask, Rng &noise, uint64_t *out) {
    for (int r = 0; r < 2; r++)
        for (int n = 0; n < POLY_N; n++) out[r * 2 * POLY_N + n] = mask.next() & GRID_MASK;
    const uint64_t *const m[2] = {out, out + 2 * POLY_N};
    uint64_t *const b[2] = {out + POLY_N, out + 3 * POLY_N};
    ggsw_bodies(ck, msg, noise, m, b);
}
// One row of a GLWE keyswitch key towards the secret `sk` (packing key, re-key key): a mask on the grid and
// body = mask (*) sk + noise + (msg << shift), rounded to the grid.  2048 draws of `mask`, then 2048 of `noise`.
void keyswitch_key_row(Rng &mask_rng, Rng &noise, const uint64_t *sk, const uint64_t *msg, int shift, uint64_t *mask,
                       uint64_t *body) {
    std::vector<uint64_t> prod(POLY_N);
    for (int n = 0; n < POLY_N; n++) mask[n] = mask_rng.next() & GRID_MASK;
    mul_binary(mask, sk, prod.data());
    for (int n = 0; n < POLY_N; n++) body[n] = round_to_grid(prod[n] + noise.noise(GLWE_NOISE) + (msg[n] << shift), BSK_QUANT_BITS);
}

void keygen(fhs_client *ck) {
    Rng r(ck->key, 1, DOM_SECRET);
    ck->lwe_sk.resize(LWE_N);
    ck->glwe_sk.resize(POLY_N);
    for (auto &b : ck->lwe_sk) b = r.next() >> 63;
    for (auto &b : ck->glwe_sk) b = r.next() >> 63;
    ck->bsk.assign((size_t)LWE_N * 4 * POLY_N, 0);
    ck->ksk.assign((size_t)BIG_N * KS_LEVEL * SMALL_CT, 0);
    // bootstrapping key: GGSW_i(lwe_sk[i])
    parallel_for(LWE_N, host_threads(32), 1, [&](size_t i) {
        Rng g(ck->key, 1000 + i, DOM_MASK), e(ck->key, 1000 + i, DOM_NOISE);
        ggsw_encrypt(ck, ck->lwe_sk[i], g, e, ck->bsk.data() + i * 4 * POLY_N);
    });
    // keyswitching key: ksk[i][l] = LWE_small(glwe_sk[i] * 2^(64 - 3(l+1)))
    parallel_for(BIG_N, host_threads(32), 1, [&](size_t i) {
        Rng g(ck->key, 100000 + i, DOM_MASK), e(ck->key, 100000 + i, DOM_NOISE);
        for (int l = 0; l < KS_LEVEL; l++) {
            uint64_t *ct = ck->ksk.data() + (i * KS_LEVEL + l) * SMALL_CT;
            uint64_t acc = 0;
            for (int j = 0; j < LWE_N; j++) {
                ct[j] = g.next();
                acc += ct[j] * ck->lwe_sk[j];
            }
            ct[LWE_N] = acc + e.noise(LWE_NOISE) + (ck->glwe_sk[i] << (64 - KS_BASE_LOG * (l + 1)));
        }
    });
}

// Pair key of the two-bits-per-product blind rotation (fftmb_kernels.hip): for every pair (s, s') = (lwe_sk[2p],
// lwe_sk[2p+1]) three GGSWs, of s(1-s'), (1-s)s' and s s', with the bootstrapping key's own parameters (GLWE noise, one
// level of base 2^23, 58-bit grid) and their own mask / noise streams.
void keygen_mb2(fhs_client *ck) {
    ck->bsk_mb2.assign((size_t)(LWE_N / 2) * 3 * 4 * POLY_N, 0);
    parallel_for((LWE_N / 2) * 3, host_threads(32), 1, [&](size_t g) {
        const size_t p = g / 3, t = g % 3;
        const uint64_t s1 = ck->lwe_sk[2 * p], s2 = ck->lwe_sk[2 * p + 1];
        const uint64_t msg = t == 0 ? s1 & (1 - s2) : t == 1 ? (1 - s1) & s2 : s1 & s2;
        Rng gm(ck->key, 2000000 + g, DOM_MASK), e(ck->key, 2000000 + g, DOM_NOISE);
        ggsw_encrypt(ck, msg, gm, e, ck->bsk_mb2.data() + g * 4 * POLY_N);
    });
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
// FHS_CLIENT_THREADS overrides the machine's count (tests: 1 = sequential).
template <class F>
void for_each_char(size_t n, F &&f) {
    size_t hw = host_threads(32);
    if (const char *e = std::getenv("FHS_CLIENT_THREADS")) hw = (size_t)std::max(1, std::atoi(e));
    parallel_for(n, std::min(hw, n / 32), 16, f);
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

int fhs_client_save(const fhs_client *ck, const char *path, int server_key_only) {
    if (!ck || !path) return FHS_ERR_ARG;
    KeyFileWriter w(path, server_key_only ? 2 : 1);
    if (!server_key_only)
        w.put(&ck->seed, 8).put(ck->lwe_sk.data(), ck->lwe_sk.size() * 8).put(ck->glwe_sk.data(), ck->glwe_sk.size() * 8);
    return w.put(ck->bsk.data(), ck->bsk.size() * 8).put(ck->ksk.data(), ck->ksk.size() * 8).close();
}

// kind 3: the pair key of the two-key-bits-per-product arithmetics alone (it accompanies a kind 1 / kind 2 file)
int fhs_client_save_multibit_key(fhs_client *ck, const char *path) {
    if (!ck || !path) return FHS_ERR_ARG;
    const uint64_t *mb = fhs_client_bsk_mb2(ck);
    return KeyFileWriter(path, 3).put(mb, FHS_BSK_MB2_WORDS * 8).close();
}

int fhs_client_load(const char *path, fhs_client **out) {
    if (!path || !out) return FHS_ERR_ARG;
    fhs_client *ck = new (std::nothrow) fhs_client();
    if (!ck) return FHS_ERR_STATE;
    KeyFileReader r(path, {1});
    r.get(&ck->seed, 8).get(ck->lwe_sk, LWE_N).get(ck->glwe_sk, POLY_N).get(ck->bsk, (size_t)LWE_N * 4 * POLY_N)
        .get(ck->ksk, (size_t)BIG_N * KS_LEVEL * SMALL_CT);
    // like the other reader of kinds 1 and 2, this one accepts trailing bytes (keyfile.h).
    // A loaded client never replays an encryption stream: fresh OS entropy for masks and noise
    if (r.finish(false) != FHS_OK || !os_entropy(&ck->key, sizeof(ck->key))) {
        delete ck;
        return FHS_ERR_STATE;
    }
    ck->enc_mask = Rng(ck->key, 7, DOM_MASK);
    ck->enc_noise = Rng(ck->key, 7, DOM_NOISE);
    *out = ck;
    return FHS_OK;
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
//   for call < 2^38; the compressed server key: 4000000 + i (BSK, key bit i), 5000000 + i (KSK, row i).  Seeded select
//   queries: SSEL_NOISE_BASE + (call << 7) + 4 bit + row, [2^63 + 2^62, 2^64) for call < 2^55.
constexpr uint64_t CSTR_STREAM_BASE = 1ull << 63;
constexpr uint64_t SSEL_NOISE_BASE = (1ull << 63) + (1ull << 62);
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
    const ChaKey seed = ck->cseed;
    // BSK: the rows of keygen's GGSW_i(lwe_sk[i]) with seeded masks, one stream per row; only the bodies are kept
    for_each_char(LWE_N, [&](size_t i) {
        std::vector<uint64_t> masks(2 * POLY_N);
        Rng e(ck->key, CBSK_NOISE_BASE + i, DOM_NOISE);
        for (int row = 0; row < 2; row++) {
            Rng g(seed, 2 * i + row, FHS_DOM_SEEDED_BSK);
            for (int n = 0; n < POLY_N; n++) masks[row * POLY_N + n] = g.next() & GRID_MASK;
        }
        const uint64_t *const m[2] = {masks.data(), masks.data() + POLY_N};
        uint64_t *const b[2] = {ck->cbsk_bodies.data() + i * 2 * POLY_N, ck->cbsk_bodies.data() + (i * 2 + 1) * POLY_N};
        ggsw_bodies(ck, ck->lwe_sk[i], e, m, b);
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
    return KeyFileWriter(path, 4).put(ck->cseed.w, 32).put(ck->cbsk_bodies.data(), FHS_CBSK_BODY_WORDS * 8)
        .put(ck->cksk_bodies.data(), FHS_CKSK_BODY_WORDS * 8).close();
}

int fhs_expand_compressed_server_key(const uint32_t seed[8], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies,
                                     uint64_t *bsk, uint64_t *ksk) {
    if (!seed || !bsk_bodies || !ksk_bodies || !bsk || !ksk) return FHS_ERR_ARG;
    const ChaKey k = seed_key(seed);
    for_each_char((size_t)LWE_N * 2, [&](size_t p) {          // GGSW row p = 2i + r
        uint64_t *mask = bsk + p * 2 * POLY_N;
        Rng g(k, p, FHS_DOM_SEEDED_BSK);
        for (int n = 0; n < POLY_N; n++) mask[n] = g.next() & GRID_MASK;
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
    parallel_for(FHS_PACK_TREE_LEVELS, FHS_PACK_TREE_LEVELS, 1, [&](size_t k) {   // one thread per tree level
        const int lv = (int)k + 1;
        const uint32_t g = (1u << lv) + 1;
        std::vector<uint64_t> sg(POLY_N);
        for (uint32_t i = 0; i < (uint32_t)POLY_N; i++) {          // S(X^g): coefficient i goes to i g mod 2N
            const uint32_t r = (i * g) & (2 * POLY_N - 1);
            sg[r & (POLY_N - 1)] = r >= (uint32_t)POLY_N ? (uint64_t)0 - ck->glwe_sk[i] : ck->glwe_sk[i];
        }
        for (int l = 0; l < FHS_PACK_LEVELS; l++) {
            const uint64_t sid = PACK_STREAM_BASE + (uint64_t)FHS_PACK_LEVELS * (lv - 1) + l;
            Rng gm(ck->key, sid, DOM_MASK), e(ck->key, sid, DOM_NOISE);
            uint64_t *mask = ck->pack_key.data() + (((size_t)(lv - 1) * FHS_PACK_LEVELS + l) * 2) * POLY_N;
            keyswitch_key_row(gm, e, ck->glwe_sk.data(), sg.data(), 64 - FHS_PACK_BASE_LOG * (l + 1), mask, mask + POLY_N);
        }
    });
}

// phases of the coefficients [lo, hi) of one packed group: ph[n - lo] = (body16[n - lo] << 48) - ((mask16 << 48) (*) S)[n];
// body16 points at the body of coefficient lo
void packed_phases(const fhs_client *ck, const uint16_t *mask16, const uint16_t *body16, size_t lo, size_t hi, uint64_t *ph) {
    std::vector<uint64_t> a(POLY_N), prod(POLY_N);
    for (int i = 0; i < POLY_N; i++) a[i] = (uint64_t)mask16[i] << 48;
    mul_binary(a.data(), ck->glwe_sk.data(), prod.data());
    for (size_t n = lo; n < hi; n++) ph[n - lo] = ((uint64_t)body16[n - lo] << 48) - prod[n];
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
    return KeyFileWriter(path, 5).put(k, FHS_PACK_KEY_WORDS * 8).close();
}

int fhs_client_encrypt_blocks(fhs_client *ck, const uint8_t *values, size_t n, uint64_t *blocks) {
    if (!ck || (n && (!values || !blocks))) return FHS_ERR_ARG;
    for (size_t i = 0; i < n; i++) encrypt_block(ck, values[i] & 31, blocks + i * BIG_CT);
    return FHS_OK;
}

int fhs_client_decrypt_packed_blocks_at(const fhs_client *ck, const void *mask16_, const void *body16_, uint32_t first_coef,
                                        size_t n_blocks, uint8_t *out) {
    const uint16_t *mask16 = static_cast<const uint16_t *>(mask16_), *body16 = static_cast<const uint16_t *>(body16_);
    if (!ck || (first_coef & 3) || first_coef >= FHS_PACK_GROUP || (n_blocks && (!mask16 || !body16 || !out))) return FHS_ERR_ARG;
    std::vector<uint64_t> ph(FHS_PACK_GROUP);
    // block i is coefficient (first_coef + i) % 2048 of mask (first_coef + i) / 2048
    const size_t end = first_coef + n_blocks;
    for (size_t g = 0; g * FHS_PACK_GROUP < end && n_blocks; g++) {
        const size_t base = g * FHS_PACK_GROUP, lo = g ? 0 : first_coef, hi = std::min<size_t>(FHS_PACK_GROUP, end - base);
        const size_t i0 = base + lo - first_coef;                    // the window's block at coefficient lo
        packed_phases(ck, mask16 + g * POLY_N, body16 + i0, lo, hi, ph.data());
        for (size_t j = 0; j < hi - lo; j++) out[i0 + j] = (uint8_t)(((ph[j] + (1ull << (DELTA_LOG - 1))) >> DELTA_LOG) & 31);
    }
    return FHS_OK;
}

int fhs_client_decrypt_packed_blocks(const fhs_client *ck, const void *mask16, const void *body16, size_t n_blocks,
                                     uint8_t *out) {
    return fhs_client_decrypt_packed_blocks_at(ck, mask16, body16, 0, n_blocks, out);
}

int fhs_client_decrypt_packed_str_at(const fhs_client *ck, const void *mask16, const void *body16, uint32_t first_coef,
                                     size_t n_chars, char *out, size_t *out_len) {
    if (!ck || !out || !out_len || (n_chars && (!mask16 || !body16))) return FHS_ERR_ARG;
    std::vector<uint8_t> blk(4 * n_chars);
    if (int rc = fhs_client_decrypt_packed_blocks_at(ck, mask16, body16, first_coef, 4 * n_chars, blk.data())) return rc;
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

int fhs_client_decrypt_packed_str(const fhs_client *ck, const void *mask16, const void *body16, size_t n_chars,
                                  char *out, size_t *out_len) {
    return fhs_client_decrypt_packed_str_at(ck, mask16, body16, 0, n_chars, out, out_len);
}

}  // extern "C"

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
    return KeyFileWriter(path, 6).put(ck->pk_seed.w, 32).put(ck->pk_body.data(), POLY_N * 8).close();
}

}  // extern "C"

// ---- string store: re-key keys (rekey_host.cpp, rekey_kernels.hip) ---------------------------------------------------
namespace {

// K[l] = (mask, body = mask (*) S_to + e + S_from 2^(64 - 16 (l + 1))) on the 58-bit grid.  Masks and noise come from a
// ChaCha key of this call alone, streams l of DOM_MASK / DOM_NOISE: OS entropy, or for an insecure seeded `to` its seed,
// the tag below and the number of keys made into it so far -- keys from different `from` clients into one `to` differ in
// their randomness whatever the clients' own generator keys are.
constexpr uint64_t SEED_TAG_REKEY = 0x5345454452454b31ull;
bool rekey_key(fhs_client *from, fhs_client *to, uint64_t *out) {
    ChaKey key;
    if (!public_seed(to, SEED_TAG_REKEY, to->rekey_calls.fetch_add(1), key)) return false;
    for (int l = 0; l < FHS_REKEY_LEVELS; l++) {
        Rng gm(key, l, DOM_MASK), e(key, l, DOM_NOISE);
        uint64_t *mask = out + (size_t)l * 2 * POLY_N;
        keyswitch_key_row(gm, e, to->glwe_sk.data(), from->glwe_sk.data(), 64 - FHS_REKEY_BASE_LOG * (l + 1), mask, mask + POLY_N);
    }
    return true;
}

}  // namespace

extern "C" {

int fhs_client_rekey_key(fhs_client *from, fhs_client *to, uint64_t *key_out) {
    if (!from || !to || !key_out) return FHS_ERR_ARG;
    return rekey_key(from, to, key_out) ? FHS_OK : FHS_ERR_STATE;
}

// kind 7: the re-key key alone
int fhs_client_save_rekey_key(fhs_client *from, fhs_client *to, const char *path) {
    if (!from || !to || !path) return FHS_ERR_ARG;
    std::vector<uint64_t> k(FHS_REKEY_KEY_WORDS);
    if (!rekey_key(from, to, k.data())) return FHS_ERR_STATE;
    return KeyFileWriter(path, 7).put(k.data(), FHS_REKEY_KEY_WORDS * 8).close();
}

}  // extern "C"

// ---- string store: select queries (select_host.cpp, select_kernels.hip) -----------------------------------------------
namespace {

// GGSW(bit) per index bit under the client's own GLWE key, four rows of keyswitch_key_row on the 58-bit grid: rows 0, 1
// carry bit (-S) 2^(64 - 16 (l + 1)) and meet the digits of a mask difference, rows 2, 3 carry bit 2^(64 - 16 (l + 1)) at
// coefficient 0 and meet the digits of a body difference.  Masks and noise come from a ChaCha key of this call alone,
// streams 4 k + row of DOM_MASK / DOM_NOISE: OS entropy, or for an insecure seeded client its seed, the tag below and the
// number of queries it has made so far.
constexpr uint64_t SEED_TAG_SELECT = 0x5345454453454c31ull;
bool select_query(fhs_client *ck, uint64_t index, int bits, uint64_t *out) {
    ChaKey key;
    if (!public_seed(ck, SEED_TAG_SELECT, ck->select_calls.fetch_add(1), key)) return false;
    std::vector<uint64_t> msg(POLY_N);
    for (int k = 0; k < bits; k++) {
        const uint64_t bit = (index >> k) & 1;
        for (int row = 0; row < 4; row++) {
            for (int n = 0; n < POLY_N; n++)
                msg[n] = row < 2 ? (uint64_t)0 - bit * ck->glwe_sk[n] : (n == 0 ? bit : 0);
            Rng gm(key, 4 * k + row, DOM_MASK), e(key, 4 * k + row, DOM_NOISE);
            uint64_t *mask = out + ((size_t)k * 4 + row) * 2 * POLY_N;
            keyswitch_key_row(gm, e, ck->glwe_sk.data(), msg.data(), 64 - 16 * ((row & 1) + 1), mask, mask + POLY_N);
        }
    }
    return true;
}

// The seeded form: the same rows with the masks drawn from the PUBLIC seed (domain FHS_DOM_SEEDED_SELECT, stream 4 k +
// row) and only the bodies kept.  The seed is public, so the noise must not come from it: it is drawn from the client's
// secret key, streams SSEL_NOISE_BASE + (call << 7) + 4 k + row (4 k + row < 96), a range of its own beside those listed
// above keygen_compressed.  The call counter is this form's own: select_calls, and with it every full-form query of an
// insecure seeded client, stays where it was.
constexpr uint64_t SEED_TAG_SELECT_SEEDED = 0x5345454453454c32ull;
bool select_query_seeded(fhs_client *ck, uint64_t index, int bits, uint32_t seed_out[8], uint64_t *bodies) {
    const uint64_t call = ck->sselect_calls.fetch_add(1);
    ChaKey seed;
    if (!public_seed(ck, SEED_TAG_SELECT_SEEDED, call, seed)) return false;
    std::vector<uint64_t> msg(POLY_N), mask(POLY_N);
    for (int k = 0; k < bits; k++) {
        const uint64_t bit = (index >> k) & 1;
        for (int row = 0; row < 4; row++) {
            for (int n = 0; n < POLY_N; n++)
                msg[n] = row < 2 ? (uint64_t)0 - bit * ck->glwe_sk[n] : (n == 0 ? bit : 0);
            Rng gm(seed, 4 * k + row, FHS_DOM_SEEDED_SELECT), e(ck->key, SSEL_NOISE_BASE + (call << 7) + 4 * k + row, DOM_NOISE);
            keyswitch_key_row(gm, e, ck->glwe_sk.data(), msg.data(), 64 - 16 * ((row & 1) + 1), mask.data(),
                              bodies + ((size_t)k * 4 + row) * POLY_N);
        }
    }
    for (int i = 0; i < 8; i++) seed_out[i] = seed.w[i];
    return true;
}

}  // namespace

extern "C" {

int fhs_client_select_query(fhs_client *ck, uint64_t index, int bits, uint64_t *query_out) {
    if (!ck || !query_out || bits < 1 || bits > 24) return FHS_ERR_ARG;
    return select_query(ck, index, bits, query_out) ? FHS_OK : FHS_ERR_STATE;
}

int fhs_client_select_query_seeded(fhs_client *ck, uint64_t index, int bits, uint32_t seed_out[8], uint64_t *bodies) {
    if (!ck || !seed_out || !bodies || bits < 1 || bits > 24) return FHS_ERR_ARG;
    return select_query_seeded(ck, index, bits, seed_out, bodies) ? FHS_OK : FHS_ERR_STATE;
}

int fhs_expand_select_query(const uint32_t seed[8], const uint64_t *bodies, int bits, uint64_t *query_out) {
    if (!seed || !bodies || !query_out || bits < 1 || bits > 24) return FHS_ERR_ARG;
    const ChaKey k = seed_key(seed);
    for (int r = 0; r < 4 * bits; r++) {                          // GGSW row r = 4 bit + row
        uint64_t *mask = query_out + (size_t)r * 2 * POLY_N;
        Rng g(k, (uint64_t)r, FHS_DOM_SEEDED_SELECT);
        for (int n = 0; n < POLY_N; n++) mask[n] = g.next() & GRID_MASK;
        std::memcpy(mask + POLY_N, bodies + (size_t)r * POLY_N, POLY_N * 8);
    }
    return FHS_OK;
}

}  // extern "C"
