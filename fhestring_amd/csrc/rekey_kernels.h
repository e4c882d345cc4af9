// Device side of the string store's re-key (rekey_kernels.hip; host reference: rekey_host.cpp).
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

hipError_t prepare_device_for_rekey();   // dynamic LDS above 64 KB, per device
hipError_t launch_rekey_glwe(const RekeyParams &p, hipStream_t s);

}  // namespace fhs
