// Host reference of the string store's select by encrypted index (include/fhestring_hip.h, "fetching a row by encrypted
// index"): a tree of CMuxes over the groups of an entry, then rotate-CMuxes inside the last group,
// every one the external product of a 32-bit GLWE difference with the GGSW of one index bit, in exact arithmetic over
// Z_2^64[X]/(X^2048+1) -- the keyswitch sum of rekey_host.cpp with four digit polynomials.  Public data only, no GPU: the
// comparator of select_kernels.hip and what CPU-only tests decrypt.
#include <algorithm>
#include <vector>

#include "../../include/fhestring_hip.h"
#include "host_ntt.h"
#include "host_parallel.h"
#include "select_kernels.h"
#include "storage_words.h"

namespace {

using namespace fhs;
constexpr int N = POLY_N;
constexpr int L = SELECT_DIGITS;
static_assert(FHS_SELECT_QUERY_BIT_WORDS == SELECT_BIT_POLYS * POLY_N && FHS_SELECT_MAX_ROW_CHARS == SELECT_MAX_ROW_CHARS &&
                  FHS_SELECT_REKEY_COST == SELECT_REKEY_COST && KEYSWITCH_BASE_LOG == 16,
              "the header's constants are the device's");

// a GLWE of 32-bit words with every body present (the ones an entry does not store are 0)
struct Glwe {
    std::vector<uint32_t> w = std::vector<uint32_t>((size_t)2 * N, 0u);
    uint32_t *mask() { return w.data(); }
    uint32_t *body() { return w.data() + N; }
    const uint32_t *mask() const { return w.data(); }
    const uint32_t *body() const { return w.data() + N; }
};

// out = round32((a << 32) + sum over the four digit polynomials of D = b - a of d (*) GGSW.row), both columns
Glwe cmux(const uint64_t *ggsw_ntt, const Glwe &a, const Glwe &b) {
    std::vector<int64_t> d((size_t)N * L);
    for (int n = 0; n < N; n++) {
        decompose((uint64_t)(b.mask()[n] - a.mask()[n]) << 32, 2, d.data() + (size_t)n * L);
        decompose((uint64_t)(b.body()[n] - a.body()[n]) << 32, 2, d.data() + (size_t)n * L + 2);
    }
    std::vector<uint64_t> ks((size_t)2 * N);
    keyswitch_sums(ggsw_ntt, L, d.data(), ks.data(), ks.data() + N);
    Glwe out;
    for (int n = 0; n < 2 * N; n++) out.w[n] = round32(((uint64_t)a.w[n] << 32) + ks[n]);
    return out;
}

// X^-s a: coefficient n is a_(n + s), negated where n + s wraps
Glwe rotated(const Glwe &a, int s) {
    Glwe b;
    for (int n = 0; n < N; n++) {
        const int m = (n + s) & (N - 1);
        const bool neg = n + s >= N;
        b.mask()[n] = neg ? 0u - a.mask()[m] : a.mask()[m];
        b.body()[n] = neg ? 0u - a.body()[m] : a.body()[m];
    }
    return b;
}

}  // namespace

extern "C" {

int fhs_store_select_bits(size_t n_chars, size_t row_chars) {
    SelectShape s;
    return select_shape(n_chars, row_chars, s) ? s.bits : 0;
}

int fhs_store_select_host(const uint64_t *query, int bits, const void *mask32_, const void *body32_, size_t n_blocks_entry,
                          size_t row_chars, void *mask32_out_, void *body32_out_) {
    const uint32_t *mask32 = static_cast<const uint32_t *>(mask32_), *body32 = static_cast<const uint32_t *>(body32_);
    uint32_t *mask_out = static_cast<uint32_t *>(mask32_out_), *body_out = static_cast<uint32_t *>(body32_out_);
    SelectShape sh;
    if (!query || !mask32 || !body32 || !mask_out || !body_out || (n_blocks_entry & 3) ||
        !select_shape(n_blocks_entry / 4, row_chars, sh) || bits != sh.bits)
        return FHS_ERR_ARG;
    const std::vector<uint64_t> query_ntt = key_to_ntt(query, (size_t)bits * SELECT_BIT_POLYS);
    auto ggsw = [&](int bit) { return query_ntt.data() + (size_t)bit * SELECT_BIT_POLYS * 2 * N; };
    std::vector<Glwe> level(sh.groups);
    for (size_t g = 0; g < sh.groups; g++) {
        const size_t count = std::min<size_t>(SELECT_GROUP, n_blocks_entry - g * SELECT_GROUP);
        std::copy(mask32 + g * N, mask32 + (g + 1) * N, level[g].mask());
        std::copy(body32 + g * SELECT_GROUP, body32 + g * SELECT_GROUP + count, level[g].body());
    }
    const Glwe zero;
    for (int t = 0; t < sh.tree_levels; t++) {                       // level t pairs nodes (2i, 2i + 1) under bit r + t
        std::vector<Glwe> next((level.size() + 1) / 2);
        parallel_for(next.size(), host_threads(16), 1, [&](size_t i) {
            next[i] = cmux(ggsw(sh.rot_bits + t), level[2 * i], 2 * i + 1 < level.size() ? level[2 * i + 1] : zero);
        });
        level.swap(next);
    }
    Glwe g = std::move(level[0]);
    for (int k = 0; k < sh.rot_bits; k++) g = cmux(ggsw(k), g, rotated(g, (int)(sh.row_blocks << k)));
    std::copy(g.mask(), g.mask() + N, mask_out);
    std::copy(g.body(), g.body() + sh.row_blocks, body_out);
    return FHS_OK;
}

}  // extern "C"
