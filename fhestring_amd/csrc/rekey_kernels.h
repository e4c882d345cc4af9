// Device side of the string store's re-key (rekey_kernels.hip; host reference: rekey_host.cpp; DESIGN.md sections 14, 16, 17).
#pragma once
#include "pbs_kernels.h"

namespace fhs {

constexpr int REKEY_LEVELS = 2;         // FHS_REKEY_LEVELS digits of
constexpr int REKEY_BASE_LOG = 16;      // FHS_REKEY_BASE_LOG bits
constexpr int REKEY_GROUP = POLY_N;     // blocks per GLWE of an entry
constexpr size_t REKEY_KEY_POLYS = (size_t)REKEY_LEVELS * 2;

// `groups` = ceil(total / 2048) groups of an entry in the compact format: mask32[groups][2048], body32[total] (group g's
// bodies start at 2048 g).  dst may be src: see the kernel.
struct RekeyParams {
    const uint32_t *src_mask, *src_body;
    uint32_t *dst_mask, *dst_body;
    uint32_t total;          // blocks of all groups together
    int groups;
    const double *key_ntt;   // [2][col 2][prime 2][16][64 lanes][2], pre-scaled by N^-1 (convert_polys_to_ntt)
    NttTables tw;
};

// The packed download for a recipient: `groups` level-11 GLWEs of the packing tree, src[groups][mask, body][2048] u64, to
// the packed format under the new key: dst_mask[groups][2048], dst_body[total] (group g's bodies start at 2048 g).
struct RekeyPackedParams {
    const uint64_t *src;
    uint16_t *dst_mask, *dst_body;
    uint32_t total;
    int groups;
    const double *key_ntt;   // as RekeyParams
    NttTables tw;
};

// The packed download of a parked entry for a recipient: `groups` covering groups of an entry in
// the compact format, to the windowed packed format under the new key.  Coefficient c = 2048 g + n of covering group g
// belongs to the window when first_coef <= c < first_coef + body_words; src_body[c] is its body word (src_body points at
// the body of coefficient 0 of the FIRST covering group, which lies inside the entry) and dst_body[c - first_coef]
// receives it.  Every mask word of every covering group is written.
struct RekeyEntryPackedParams {
    const uint32_t *src_mask, *src_body;
    uint16_t *dst_mask, *dst_body;
    uint32_t first_coef;     // < 2048
    uint32_t body_words;     // blocks of the window, > 0
    int groups;              // ceil((first_coef + body_words) / 2048)
    const double *key_ntt;   // as RekeyParams
    NttTables tw;
};

hipError_t prepare_device_for_rekey();   // dynamic LDS above 64 KB, per device
hipError_t launch_rekey_glwe(const RekeyParams &p, hipStream_t s);
hipError_t launch_rekey_packed(const RekeyPackedParams &p, hipStream_t s);
hipError_t launch_rekey_entry_packed(const RekeyEntryPackedParams &p, hipStream_t s);

}  // namespace fhs
