// Device side of the string store's select by encrypted index (select_kernels.hip; host reference: select_host.cpp;
// DESIGN.md section 23), and the geometry that host and device share.
#pragma once
#include "pbs_kernels.h"

namespace fhs {

constexpr int SELECT_DIGITS = 4;             // two 16-bit digits of the mask difference, then two of the body difference
constexpr int SELECT_GROUP = POLY_N;         // blocks per GLWE of an entry
constexpr int SELECT_MAX_ROW_CHARS = 512;    // FHS_SELECT_MAX_ROW_CHARS: a row never spans two groups
constexpr size_t SELECT_BIT_POLYS = (size_t)SELECT_DIGITS * 2;   // polynomials of one GGSW: FHS_SELECT_QUERY_BIT_WORDS / 2048
// re-key units one CMux is charged with: ceil(sigma_cmux^2 / sigma_rekey^2) = ceil(1.03)
constexpr int SELECT_REKEY_COST = 2;         // FHS_SELECT_REKEY_COST

// An entry of n_chars characters read as R = n_chars / row_chars rows.  A row is 4 row_chars consecutive blocks, a group
// of 2048 blocks holds 2^r of them.  Index bit k < rot_bits rotates inside the last group, bit rot_bits + t is level t of
// the tree over the groups.  With one group there is no tree and only ceil(log2 R) rotate bits exist.
struct SelectShape {
    size_t rows = 0, groups = 0, row_blocks = 0;
    int r = 0, rot_bits = 0, tree_levels = 0, bits = 0;
};
inline int ceil_log2(size_t x) {
    int b = 0;
    while (((size_t)1 << b) < x) b++;
    return b;
}
// false for a refused shape: row_chars not a power of two in 1..512, n_chars not a multiple of it, fewer than two rows
inline bool select_shape(size_t n_chars, size_t row_chars, SelectShape &s) {
    if (row_chars == 0 || row_chars > (size_t)SELECT_MAX_ROW_CHARS || (row_chars & (row_chars - 1))) return false;
    if (n_chars % row_chars || n_chars / row_chars < 2 || n_chars > ((size_t)1 << 24)) return false;
    s.rows = n_chars / row_chars;
    s.row_blocks = 4 * row_chars;
    s.groups = (4 * n_chars + SELECT_GROUP - 1) / SELECT_GROUP;
    s.r = ceil_log2(SELECT_GROUP / s.row_blocks);
    s.bits = ceil_log2(s.rows);
    s.rot_bits = s.groups == 1 ? s.bits : s.r;
    s.tree_levels = s.bits - s.rot_bits;      // = ceil(log2 groups)
    return true;
}

// GLWEs of one query in the level buffer `which` (0: launches 0, 2, ..; 1: launches 1, 3, ..)
inline size_t select_ws_nodes(const SelectShape &s, int which) {
    return which ? (s.groups + 3) / 4 > 1 ? (s.groups + 3) / 4 : 1 : (s.groups + 1) / 2 > 1 ? (s.groups + 1) / 2 : 1;
}

// One launch: a tree level (rotate == 0: workgroup i is the CMux of source nodes 2i and 2i + 1 under GGSW `bit`; a node
// past src_nodes is the zero GLWE) or a rotate bit (rotate = s > 0: workgroup i is CMux(a, X^-s a) of source node i).
// Source and destination have the entry's layout, mask[nodes][2048] and body[nodes][2048]: node k of the source has
// min(2048, src_body_total - 2048 k) body words, the ones it does not store count as 0 (the tail of an entry's last
// group); every destination node receives 2048 mask words and its first store_body body words.  Never in place.
struct SelectCmuxParams {
    const uint32_t *src_mask, *src_body;
    uint32_t src_nodes;        // > 0
    uint32_t src_body_total;   // ceil(src_body_total / 2048) == src_nodes
    uint32_t rotate;           // 0, or 0 < s < 2048
    uint32_t *dst_mask, *dst_body;
    uint32_t store_body;       // 1..2048
    const double *query_ntt;   // [bits][4][col 2][prime 2][16][64 lanes][2], pre-scaled by N^-1 (convert_polys_to_ntt)
    int bit;
    NttTables tw;
    // Several queries in one launch: query y (blockIdx.y) reads src_mask / src_body + y src_stride (0 while every query
    // reads the entry itself), writes dst_mask / dst_body + y dst_stride and uses query_ntt + y query_stride.  With a
    // dst_table (one destination node only) it writes mask[2048] | body at dst_table[y] instead: the new entries.
    uint32_t queries;          // > 0
    size_t src_stride, dst_stride;   // 32-bit words
    size_t query_stride;             // doubles
    uint32_t *const *dst_table;      // device array [queries], or null
};

// select_query_to_ntt_kernel: n_polys polynomials to query_ntt's layout, out[poly][prime][16][64 lanes][2], the doubles
// of convert_polys_to_ntt(words, out, n_polys, quant_bits) bit for bit.  seeds == null: words[n_polys][2048].  Otherwise
// the seeded form of queries of query_polys polynomials each (8 per index bit): polynomial 2 r of query i is the mask of
// GGSW row r, drawn in the kernel from seeds[i][8] (domain FHS_DOM_SEEDED_SELECT, stream r), polynomial 2 r + 1 its body,
// words[i][query_polys / 2][2048].
struct SelectQueryParams {
    const uint64_t *words;
    const uint32_t *seeds;
    uint32_t n_polys, query_polys;
    int quant_bits;            // 1..32
    double *out;
    NttTables tw;
};

hipError_t prepare_device_for_select();   // dynamic LDS above 64 KB, per device, both kernels
hipError_t launch_select_cmux(const SelectCmuxParams &p, hipStream_t s);
hipError_t launch_select_query_to_ntt(const SelectQueryParams &p, hipStream_t s);

}  // namespace fhs
