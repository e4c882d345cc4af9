// Host reference of the packed result download (include/fhestring_hip.h, "packed result download"):
// ring packing of up to 2048 LWE blocks into one GLWE (Chen, Dai, Kim, Song, Alg. PackLWEs) in exact arithmetic over
// Z_2^64[X]/(X^2048+1).  Public data only, no GPU: the comparator of pack_kernels.hip and what CPU-only tests decrypt.
// The negacyclic products run through the host NTT over the device's two primes (host_ntt.h; any exact method gives the
// same words, and tests/test_packed.py checks a node against a schoolbook product that uses no transform).
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/fhestring_hip.h"
#include "host_ntt.h"
#include "host_parallel.h"
#include "pbs_kernels.h"
#include "storage_words.h"

namespace {

using namespace fhs;
constexpr int N = POLY_N;
constexpr int L = FHS_PACK_LEVELS;
static_assert(FHS_PACK_BASE_LOG == KEYSWITCH_BASE_LOG, "the packing key has the shared keyswitch's digit width");

// the packing key as residues (key_to_ntt): [11][L][mask, body][prime][2048]; one tree level's part is a keyswitch key
constexpr size_t KEY_POLYS = (size_t)FHS_PACK_TREE_LEVELS * L * 2;
const uint64_t *level_key(const std::vector<uint64_t> &key_ntt, int lv) { return key_ntt.data() + (size_t)(lv - 1) * L * 2 * 2 * N; }

// one tree node: out = P + AutoKS_g(M), T = X^t O, P = E + T, M = E - T, g = 2^lv + 1, t = N >> lv.
// e / o / out: mask[2048] | body[2048]; o == nullptr: the odd child is absent (zero).
void pack_node(const std::vector<uint64_t> &key_ntt, int lv, const uint64_t *e, const uint64_t *o, uint64_t *out) {
    const uint32_t t = (uint32_t)N >> lv, g = (1u << lv) + 1;
    std::vector<uint64_t> buf((size_t)6 * N);
    uint64_t *P = buf.data(), *A1 = P + 2 * N /* A'(X) | B'(X) */, *ks = A1 + 2 * N /* mask | body */;
    for (int c = 0; c < 2; c++)
        for (uint32_t i = 0; i < (uint32_t)N; i++) {
            uint64_t tv = 0;
            if (o) tv = i >= t ? o[c * N + i - t] : (uint64_t)0 - o[c * N + i - t + N];
            const uint64_t ev = e[c * N + i];
            P[c * N + i] = ev + tv;
            const uint64_t m = ev - tv;
            const uint32_t r = (i * g) & (2 * N - 1);                  // the automorphism X -> X^g
            A1[c * N + (r & (N - 1))] = r >= (uint32_t)N ? (uint64_t)0 - m : m;
        }
    std::vector<int64_t> d((size_t)N * L);
    for (int n = 0; n < N; n++) decompose(A1[n], L, d.data() + (size_t)n * L);
    keyswitch_sums(level_key(key_ntt, lv), L, d.data(), ks, ks + N);
    for (int c = 0; c < 2; c++)
        for (int n = 0; n < N; n++) out[c * N + n] = P[c * N + n] + (c ? A1[N + n] : 0) - ks[c * N + n];
}

// leaf GLWE of one block, pre-scaled by 1/N with rounding: A_0 = a_0, A_{N-i} = -a_i, B_0 = b
inline uint64_t prescale(uint64_t x) { return (x + (1ull << 10)) >> 11; }
void leaf_glwe(const uint64_t *blk, uint64_t *out) {
    std::memset(out, 0, 2 * N * 8);
    out[0] = prescale(blk[0]);
    for (int i = 1; i < N; i++) out[N - i] = (uint64_t)0 - prescale(blk[i]);
    out[N] = prescale(blk[BIG_N]);
}

// one group: `count` blocks (1..2048) -> mask[2048], body[2048].  Node k of level lv holds the blocks = k mod (N >> lv);
// its children at level lv - 1 are nodes k (even) and k + (N >> lv) (odd); a node is live when block k exists.
void pack_group(const std::vector<uint64_t> &key_ntt, const uint64_t *blocks, size_t count, uint64_t *mask, uint64_t *body) {
    std::vector<uint64_t> cur, prev;
    for (int lv = 1; lv <= FHS_PACK_TREE_LEVELS; lv++) {
        const size_t n_lv = (size_t)N >> lv, live = std::min(count, n_lv);
        prev.swap(cur);
        cur.assign(live * 2 * N, 0);
        parallel_for(live, host_threads(16), 1, [&](size_t k) {
            const bool has_o = k + n_lv < count;
            if (lv == 1) {
                std::vector<uint64_t> leaves(4 * N);
                leaf_glwe(blocks + k * BIG_CT, leaves.data());
                if (has_o) leaf_glwe(blocks + (k + n_lv) * BIG_CT, leaves.data() + 2 * N);
                pack_node(key_ntt, lv, leaves.data(), has_o ? leaves.data() + 2 * N : nullptr, cur.data() + k * 2 * N);
            } else {
                pack_node(key_ntt, lv, prev.data() + k * 2 * N, has_o ? prev.data() + (k + n_lv) * 2 * N : nullptr,
                          cur.data() + k * 2 * N);
            }
        });
    }
    std::memcpy(mask, cur.data(), N * 8);
    std::memcpy(body, cur.data() + N, N * 8);
}

}  // namespace

extern "C" {

void fhs_packed_bytes(size_t n_chars, size_t *mask_words, size_t *body_words) {
    const size_t nb = 4 * n_chars;
    if (mask_words) *mask_words = (nb + FHS_PACK_GROUP - 1) / FHS_PACK_GROUP * (size_t)N;
    if (body_words) *body_words = nb;
}

int fhs_pack_host(const uint64_t *key, const uint64_t *blocks, size_t n_blocks, uint64_t *mask64, uint64_t *body64) {
    if (!key || (n_blocks && (!blocks || !mask64 || !body64))) return FHS_ERR_ARG;
    const std::vector<uint64_t> key_ntt = key_to_ntt(key, KEY_POLYS);
    for (size_t g = 0; g * FHS_PACK_GROUP < n_blocks; g++)
        pack_group(key_ntt, blocks + g * FHS_PACK_GROUP * BIG_CT, std::min<size_t>(FHS_PACK_GROUP, n_blocks - g * FHS_PACK_GROUP),
                   mask64 + g * N, body64 + g * N);
    return FHS_OK;
}

int fhs_pack_switch16(const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, void *mask16_, void *body16_) {
    uint16_t *mask16 = static_cast<uint16_t *>(mask16_), *body16 = static_cast<uint16_t *>(body16_);
    if (n_blocks && (!mask64 || !body64 || !mask16 || !body16)) return FHS_ERR_ARG;
    for (size_t g = 0; g * FHS_PACK_GROUP < n_blocks; g++) {
        const size_t count = std::min<size_t>(FHS_PACK_GROUP, n_blocks - g * FHS_PACK_GROUP);
        for (int i = 0; i < N; i++) mask16[g * N + i] = round16(mask64[g * N + i]);
        for (size_t j = 0; j < count; j++) body16[g * FHS_PACK_GROUP + j] = round16(body64[g * N + j]);
    }
    return FHS_OK;
}

int fhs_pack_switch32(const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, void *mask32_, void *body32_) {
    uint32_t *mask32 = static_cast<uint32_t *>(mask32_), *body32 = static_cast<uint32_t *>(body32_);
    if (n_blocks && (!mask64 || !body64 || !mask32 || !body32)) return FHS_ERR_ARG;
    for (size_t g = 0; g * FHS_PACK_GROUP < n_blocks; g++) {
        const size_t count = std::min<size_t>(FHS_PACK_GROUP, n_blocks - g * FHS_PACK_GROUP);
        for (int i = 0; i < N; i++) mask32[g * N + i] = round32(mask64[g * N + i]);
        for (size_t j = 0; j < count; j++) body32[g * FHS_PACK_GROUP + j] = round32(body64[g * N + j]);
    }
    return FHS_OK;
}

int fhs_debug_pack_node(const uint64_t *key, int lv, const uint64_t *e, const uint64_t *o, uint64_t *out) {
    if (!key || !e || !o || !out || lv < 1 || lv > FHS_PACK_TREE_LEVELS) return FHS_ERR_ARG;
    const std::vector<uint64_t> key_ntt = key_to_ntt(key, KEY_POLYS);
    pack_node(key_ntt, lv, e, o, out);
    return FHS_OK;
}

}  // extern "C"
