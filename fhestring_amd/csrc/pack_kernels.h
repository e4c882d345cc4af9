// Device side of the packed result download (pack_kernels.hip; host reference: pack_host.cpp).
#pragma once
#include "pbs_kernels.h"

namespace fhs {

constexpr int PACK_LEVELS = 3;          // FHS_PACK_LEVELS digits of
constexpr int PACK_BASE_LOG = 16;       // FHS_PACK_BASE_LOG bits
constexpr int PACK_TREE_LEVELS = 11;    // log2(POLY_N)
constexpr int PACK_GROUP = POLY_N;      // blocks per packed GLWE
constexpr size_t PACK_KEY_POLYS = (size_t)PACK_TREE_LEVELS * PACK_LEVELS * 2;

// One leaf of a group: a pool block, or (blk == nullptr) the trivial block (0, body).
struct PackLeaf {
    const uint64_t *blk;
    uint64_t body;
};

// One tree level of `groups` groups (grid.y); group y holds min(2048, total - 2048 y) blocks and only its live nodes
// (node k is live when block k of the group exists) are launched.  A GLWE in the workspace is mask[2048] | body[2048].
struct PackLevelParams {
    int lv;                  // 1..11; level lv has 2048 >> lv nodes per group
    int groups;
    uint32_t total;          // blocks of all `groups` groups together
    const PackLeaf *leaves;  // lv == 1: [total]
    const uint64_t *src;     // lv > 1: [groups][2 * (2048 >> lv)][2][2048], the level below
    uint64_t *dst;           // [groups][2048 >> lv][2][2048]
    const double *key_ntt;   // [11][3][col 2][prime 2][16][64 lanes][2], pre-scaled by N^-1 (convert_polys_to_ntt)
    NttTables tw;
};

hipError_t prepare_device_for_packing();   // dynamic LDS above 64 KB, per device
hipError_t launch_pack_level(const PackLevelParams &p, hipStream_t s);
// storage switch of the level-11 GLWEs ([groups][2][2048], the layout of PackLevelParams::dst at lv == 11) to 16 bits:
// mask16[groups][2048], body16[total] (group g's bodies start at 2048 g)
hipError_t launch_pack_switch16(const uint64_t *d_glwe, uint16_t *d_mask16, uint16_t *d_body16, int groups, uint32_t total,
                                hipStream_t s);

}  // namespace fhs
