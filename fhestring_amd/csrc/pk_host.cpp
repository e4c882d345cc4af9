// Public-key string encryption and the host reference of its expansion (include/fhestring_hip.h, "public-key
// encryption").  Nothing here knows a secret key or touches a GPU: the handle holds the public RLWE
// sample (A, B = A S + E) of the client, the encryptor makes one GLWE ciphertext per 2048 blocks under it, and the
// expansion is a sample extraction per block -- the comparator of pk_kernels.hip and what CPU-only tests decrypt.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/fhestring_hip.h"
#include "chacha_rng.h"
#include "host_parallel.h"
#include "keyfile.h"
#include "pbs_kernels.h"
#include "storage_words.h"

namespace {

using namespace fhs;
using namespace fhs_rng;
constexpr int N = POLY_N;
constexpr size_t GROUP = FHS_PK_GROUP;
constexpr size_t MAX_CHARS = (size_t)1 << 24;        // the limit of fhs_client_encrypt_str

struct PublicKey {
    uint32_t seed[8];
    std::vector<uint64_t> a, b;                      // A (regenerated from the seed), B
    std::atomic<bool> insecure{false};               // fhs_public_key_set_insecure_seed (tests)
    std::atomic<uint64_t> test_seed{0}, calls{0};
};


// one group: mask = A U + E1, body = B U + E2 + messages, U binary -- both negacyclic products as sums of signed shifts
void encrypt_group(const PublicKey &pk, const ChaKey &key, uint64_t g, const uint8_t *msg, size_t count, uint32_t *mask32,
                   uint32_t *body32) {
    std::vector<uint64_t> u(N), mask(N, 0), body(N, 0);
    Rng ru(key, g, DOM_SECRET), e1(key, 2 * g, DOM_NOISE), e2(key, 2 * g + 1, DOM_NOISE);
    ru.fill(u.data(), N);
    const uint64_t *a = pk.a.data(), *b = pk.b.data();
    for (int j = 0; j < N; j++) {
        if (!(u[j] >> 63)) continue;
        for (int k = 0; k < j; k++) { mask[k] -= a[k + N - j]; body[k] -= b[k + N - j]; }
        for (int k = j; k < N; k++) { mask[k] += a[k - j]; body[k] += b[k - j]; }
    }
    for (int k = 0; k < N; k++) mask32[k] = round32(mask[k] + e1.noise(GLWE_NOISE));
    for (size_t k = 0; k < (size_t)N; k++) {
        const uint64_t x = body[k] + e2.noise(GLWE_NOISE);       // (drawn for absent blocks too: one stream layout)
        if (k < count) body32[k] = round32(x + ((uint64_t)msg[k] << DELTA_LOG));
    }
}

bool window_ok(size_t n_total, size_t first_char, size_t count) {
    return n_total <= MAX_CHARS && first_char <= n_total && count <= n_total - first_char;
}

}  // namespace

extern "C" {

int fhs_public_key_create(const uint32_t seed[8], const uint64_t *body, void **pk_out) {
    if (!seed || !body || !pk_out) return FHS_ERR_ARG;
    PublicKey *pk = new (std::nothrow) PublicKey();
    if (!pk) return FHS_ERR_STATE;
    ChaKey k;
    for (int i = 0; i < 8; i++) k.w[i] = pk->seed[i] = seed[i];
    pk->a.resize(N);
    Rng(k, 0, FHS_DOM_PUBLIC_KEY).fill(pk->a.data(), N);
    pk->b.assign(body, body + N);
    *pk_out = pk;
    return FHS_OK;
}

int fhs_public_key_load(const char *path, void **pk_out) {
    if (!path || !pk_out) return FHS_ERR_ARG;
    uint32_t seed[8];
    std::vector<uint64_t> body;
    if (fhs_read_public_key_file(path, seed, body) != FHS_OK) return FHS_ERR_STATE;
    return fhs_public_key_create(seed, body.data(), pk_out);
}

void fhs_public_key_destroy(void *pk) { delete static_cast<PublicKey *>(pk); }

int fhs_public_key_get(const void *pk_, uint32_t seed_out[8], uint64_t *body_out) {
    const PublicKey *pk = static_cast<const PublicKey *>(pk_);
    if (!pk || !seed_out || !body_out) return FHS_ERR_ARG;
    std::memcpy(seed_out, pk->seed, 32);
    std::memcpy(body_out, pk->b.data(), (size_t)N * 8);
    return FHS_OK;
}

int fhs_public_key_set_insecure_seed(void *pk_, uint64_t seed) {
    PublicKey *pk = static_cast<PublicKey *>(pk_);
    if (!pk) return FHS_ERR_ARG;
    pk->test_seed = seed;
    pk->calls = 0;
    pk->insecure = true;
    return FHS_OK;
}

void fhs_public_str_words(size_t n_chars, size_t *mask_words, size_t *body_words) {
    if (mask_words) *mask_words = (4 * n_chars + GROUP - 1) / GROUP * (size_t)N;
    if (body_words) *body_words = 4 * n_chars;
}

int fhs_public_encrypt_str(void *pk_, const char *s, size_t len, size_t padding, void *mask32_, void *body32_) {
    PublicKey *pk = static_cast<PublicKey *>(pk_);
    uint32_t *mask32 = static_cast<uint32_t *>(mask32_), *body32 = static_cast<uint32_t *>(body32_);
    if (!pk || (len && !s)) return FHS_ERR_ARG;
    for (size_t i = 0; i < len; i++)
        if ((unsigned char)s[i] >= 128 || s[i] == 0) return FHS_ERR_ARG;
    if (len > MAX_CHARS || padding > MAX_CHARS - len) return FHS_ERR_LIMIT;
    const size_t n = len + padding;
    if (n && (!mask32 || !body32)) return FHS_ERR_ARG;
    // the encryptor's own ChaCha key: fresh OS entropy per call (or the test seed and the call number)
    ChaKey key;
    if (pk->insecure) {
        const uint64_t call = pk->calls.fetch_add(1);
        key = key_from_seed(pk->test_seed ^ 0x5055424c49434b31ull);
        key.w[6] ^= (uint32_t)call;
        key.w[7] ^= (uint32_t)(call >> 32);
    } else if (!os_entropy(&key, sizeof(key))) {
        return FHS_ERR_STATE;
    }
    std::vector<uint8_t> msg(4 * n, 0);
    for (size_t i = 0; i < len; i++)
        for (int d = 0; d < 4; d++) msg[4 * i + d] = ((uint8_t)s[i] >> (2 * d)) & 3;
    parallel_for((4 * n + GROUP - 1) / GROUP, host_threads(16), 1, [&](size_t g) {
        encrypt_group(*pk, key, g, msg.data() + g * GROUP, std::min(GROUP, 4 * n - g * GROUP), mask32 + g * N,
                      body32 + g * GROUP);
    });
    return FHS_OK;
}

int fhs_expand_public_str(const void *mask32_, const void *body32_, size_t n_total, size_t first_char, size_t count,
                          uint64_t *out) {
    const uint32_t *mask32 = static_cast<const uint32_t *>(mask32_), *body32 = static_cast<const uint32_t *>(body32_);
    if (!window_ok(n_total, first_char, count) || (count && (!mask32 || !body32 || !out))) return FHS_ERR_ARG;
    const size_t t0 = 4 * first_char, nb = 4 * count;
    parallel_for((nb + 63) / 64, host_threads(16), 1, [&](size_t w) {
        for (size_t k = 64 * w; k < std::min(nb, 64 * w + 64); k++) {
            const size_t t = t0 + k;
            const uint32_t *a = mask32 + t / GROUP * N;
            const int j = (int)(t % GROUP);
            uint64_t *ct = out + k * BIG_CT;
            for (int i = 0; i <= j; i++) ct[i] = (uint64_t)a[j - i] << 32;
            for (int i = j + 1; i < N; i++) ct[i] = (uint64_t)0 - ((uint64_t)a[N + j - i] << 32);
            ct[N] = (uint64_t)body32[t] << 32;
        }
    });
    return FHS_OK;
}

}  // extern "C"
