// Launchers of store_kernels.hip: the storage switches of the device-resident string store (include/fhestring_hip.h,
// "device-resident string store").
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace fhs {

// One pass of a store entry: the level-11 GLWEs of `groups` (<= 4) packing groups ([groups][2][2048] u64, the layout of
// PackLevelParams::dst at lv == 11) holding `total` blocks together -> every word (x + 2^31) >> 32, written into the entry
// itself: group first_group + g's mask to entry_mask32[(first_group + g) * 2048 ..], its min(2048, total - 2048 g) bodies
// to entry_body32[(first_group + g) * 2048 ..].  entry_mask32 / entry_body32 are the ENTRY's bases (8-byte aligned).
hipError_t launch_store_switch32(const uint64_t *d_glwe, uint32_t *entry_mask32, uint32_t *entry_body32,
                                 uint32_t first_group, int groups, uint32_t total, hipStream_t s);

// A window of a parked entry as the packed download's 16-bit words, every word (w + 2^15) >> 16:
// mask32 = the first covering group's mask inside the entry, `groups` whole groups -> mask16[groups][2048]; body32 = the
// window's first body inside the entry, body_words = 4 x characters -> body16[body_words].  Sources 16-byte aligned (a
// window starts at a whole character), destinations 8-byte aligned; one launch.
hipError_t launch_store_switch16(const uint32_t *mask32, const uint32_t *body32, uint16_t *mask16, uint16_t *body16, int groups,
                                 size_t body_words, hipStream_t s);

}  // namespace fhs
