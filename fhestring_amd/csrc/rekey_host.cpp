// Host reference of the string store's re-key (include/fhestring_hip.h, "re-keying parked entries"; DESIGN.md section
// 14): one GLWE keyswitch per group of 2048 blocks in exact arithmetic over Z_2^64[X]/(X^2048+1) -- the AutoKS of
// pack_host.cpp without the automorphism, two digits of 16 bits on words that have 32 significant bits.  Public data
// only, no GPU: the comparator of rekey_kernels.hip and what CPU-only tests decrypt.
#include <algorithm>
#include <vector>

#include "../../include/fhestring_hip.h"
#include "host_ntt.h"
#include "host_parallel.h"
#include "pbs_kernels.h"
#include "storage_words.h"

namespace {

using namespace fhs;
constexpr int N = POLY_N;
constexpr int L = FHS_REKEY_LEVELS;
static_assert(L == 2 && FHS_REKEY_BASE_LOG == KEYSWITCH_BASE_LOG, "the digits are the two 16-bit halves of a 32-bit word");

// the 64-bit keyswitch sums of one group before any rounding (host_ntt.h): ks = mask | body [2048] each, from the mask's
// 32-bit words: a << 32 = d_0 2^48 + d_1 2^32 exactly.  Shared by all three formats below.
std::vector<uint64_t> keyswitch_sums32(const uint64_t *key_ntt, const uint32_t *a32) {
    std::vector<int64_t> d((size_t)N * L);
    for (int n = 0; n < N; n++) decompose((uint64_t)a32[n] << 32, L, d.data() + (size_t)n * L);
    std::vector<uint64_t> ks((size_t)2 * N);
    keyswitch_sums(key_ntt, L, d.data(), ks.data(), ks.data() + N);
    return ks;
}

// one group in place of (or next to) its source: mask[2048], body[count]
void rekey_group(const uint64_t *key_ntt, const uint32_t *mask, const uint32_t *body, size_t count, uint32_t *mask_out,
                 uint32_t *body_out) {
    const std::vector<uint64_t> ks = keyswitch_sums32(key_ntt, mask);                 // (every mask word is read here)
    for (int n = 0; n < N; n++) mask_out[n] = round32((uint64_t)0 - ks[n]);
    for (size_t j = 0; j < count; j++) body_out[j] = round32(((uint64_t)body[j] << 32) - ks[N + j]);
}

// one group of the packed download for a recipient: the level-11 GLWE of the packing tree, 64-bit
// words; the mask is rounded to 32 bits on the way in (fhs_pack_switch32's word), the body is not; one rounding to 16
// bits at the end (fhs_pack_switch16's word)
void rekey_packed_group(const uint64_t *key_ntt, const uint64_t *mask64, const uint64_t *body64, size_t count,
                        uint16_t *mask_out, uint16_t *body_out) {
    std::vector<uint32_t> a(N);
    for (int n = 0; n < N; n++) a[n] = round32(mask64[n]);
    const std::vector<uint64_t> ks = keyswitch_sums32(key_ntt, a.data());
    for (int n = 0; n < N; n++) mask_out[n] = round16((uint64_t)0 - ks[n]);
    for (size_t j = 0; j < count; j++) body_out[j] = round16(body64[j] - ks[N + j]);
}

// one covering group of the packed download of a parked entry: the entry's 32-bit words are the
// keyswitch's input as they are; bodies exist for the window's coefficients [lo, hi) of the group only: body32 points at
// coefficient 0 of the group and is read inside [lo, hi) alone, body_out at the output word of coefficient lo
void store_packed_group(const uint64_t *key_ntt, const uint32_t *mask32, const uint32_t *body32, size_t lo, size_t hi,
                        uint16_t *mask_out, uint16_t *body_out) {
    if (!key_ntt) {                                                  // own key: the storage switch alone
        for (int n = 0; n < N; n++) mask_out[n] = round16((uint64_t)mask32[n] << 32);
        for (size_t n = lo; n < hi; n++) body_out[n - lo] = round16((uint64_t)body32[n] << 32);
        return;
    }
    const std::vector<uint64_t> ks = keyswitch_sums32(key_ntt, mask32);
    for (int n = 0; n < N; n++) mask_out[n] = round16((uint64_t)0 - ks[n]);
    for (size_t n = lo; n < hi; n++) body_out[n - lo] = round16(((uint64_t)body32[n] << 32) - ks[N + n]);
}

}  // namespace

extern "C" {

int fhs_rekey_host(const uint64_t *key, const void *mask32_, const void *body32_, size_t n_blocks, void *mask32_out_,
                   void *body32_out_) {
    const uint32_t *mask32 = static_cast<const uint32_t *>(mask32_), *body32 = static_cast<const uint32_t *>(body32_);
    uint32_t *mask_out = static_cast<uint32_t *>(mask32_out_), *body_out = static_cast<uint32_t *>(body32_out_);
    if (!key || (n_blocks && (!mask32 || !body32 || !mask_out || !body_out))) return FHS_ERR_ARG;
    const std::vector<uint64_t> key_ntt = key_to_ntt(key, (size_t)L * 2);
    const size_t groups = (n_blocks + FHS_PACK_GROUP - 1) / FHS_PACK_GROUP;
    parallel_for(groups, host_threads(16), 1, [&](size_t g) {          // groups are independent, in place too
        const size_t count = std::min<size_t>(FHS_PACK_GROUP, n_blocks - g * FHS_PACK_GROUP);
        rekey_group(key_ntt.data(), mask32 + g * N, body32 + g * FHS_PACK_GROUP, count, mask_out + g * N,
                    body_out + g * FHS_PACK_GROUP);
    });
    return FHS_OK;
}

int fhs_rekey_packed_host(const uint64_t *key, const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, void *mask16_,
                          void *body16_) {
    uint16_t *mask16 = static_cast<uint16_t *>(mask16_), *body16 = static_cast<uint16_t *>(body16_);
    if (!key || (n_blocks && (!mask64 || !body64 || !mask16 || !body16))) return FHS_ERR_ARG;
    const std::vector<uint64_t> key_ntt = key_to_ntt(key, (size_t)L * 2);
    const size_t groups = (n_blocks + FHS_PACK_GROUP - 1) / FHS_PACK_GROUP;
    parallel_for(groups, host_threads(16), 1, [&](size_t g) {
        const size_t count = std::min<size_t>(FHS_PACK_GROUP, n_blocks - g * FHS_PACK_GROUP);
        rekey_packed_group(key_ntt.data(), mask64 + g * N, body64 + g * N, count, mask16 + g * N, body16 + g * FHS_PACK_GROUP);
    });
    return FHS_OK;
}

void fhs_store_packed_words(size_t first_char, size_t count, size_t *mask_words, size_t *body_words, uint32_t *first_coef) {
    const size_t t0 = 4 * first_char;
    if (mask_words) *mask_words = count ? ((t0 + 4 * count - 1) / FHS_PACK_GROUP - t0 / FHS_PACK_GROUP + 1) * (size_t)N : 0;
    if (body_words) *body_words = 4 * count;
    if (first_coef) *first_coef = (uint32_t)(t0 % FHS_PACK_GROUP);
}

int fhs_store_packed_host(const uint64_t *key, const void *mask32_, const void *body32_, size_t n_blocks_entry, size_t first_char,
                          size_t count, void *mask16_, void *body16_) {
    const uint32_t *mask32 = static_cast<const uint32_t *>(mask32_), *body32 = static_cast<const uint32_t *>(body32_);
    uint16_t *mask16 = static_cast<uint16_t *>(mask16_), *body16 = static_cast<uint16_t *>(body16_);
    const size_t n_chars = n_blocks_entry / 4;
    if ((n_blocks_entry & 3) || first_char > n_chars || count > n_chars - first_char) return FHS_ERR_ARG;
    if (count == 0) return FHS_OK;
    if (!mask32 || !body32 || !mask16 || !body16) return FHS_ERR_ARG;
    std::vector<uint64_t> key_ntt;
    if (key) key_ntt = key_to_ntt(key, (size_t)L * 2);
    const size_t t0 = 4 * first_char, t1 = t0 + 4 * count, g0 = t0 / FHS_PACK_GROUP, g1 = (t1 - 1) / FHS_PACK_GROUP;
    parallel_for(g1 - g0 + 1, host_threads(16), 1, [&](size_t k) {
        const size_t base = (g0 + k) * FHS_PACK_GROUP;               // the group's coefficient 0 as a block of the entry
        const size_t lo = std::max(t0, base) - base, hi = std::min<size_t>(t1 - base, FHS_PACK_GROUP);
        store_packed_group(key ? key_ntt.data() : nullptr, mask32 + (g0 + k) * N, body32 + base, lo, hi, mask16 + k * N,
                           body16 + (base + lo - t0));
    });
    return FHS_OK;
}

}  // extern "C"
