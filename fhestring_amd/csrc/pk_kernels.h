// Launcher of pk_kernels.hip: sample extraction of public-key (compact) strings straight into pool blocks (the
// convention of include/fhestring_hip.h, "public-key encryption").
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace fhs {

constexpr int PK_BLOCKS_PER_WG = 8;     // consecutive blocks of one group per workgroup (one LDS staging of its mask)

// n blocks of one public-key string: pass-local block k is coefficient (first_coef + k) % 2048 of group
// (first_coef + k) / 2048 of the pass, first_coef < 2048.  d_masks = the u32 masks of the groups the pass touches
// ([groups][2048]), d_bodies[n] the blocks' u32 bodies, d_dst[n] the destination blocks (16-byte aligned, 2049 words).
hipError_t launch_expand_public_blocks(const uint32_t *d_masks, const uint32_t *d_bodies, uint64_t *const *d_dst,
                                       uint32_t first_coef, int n, hipStream_t s);

}  // namespace fhs
