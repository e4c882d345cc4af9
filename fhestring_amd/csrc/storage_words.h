// The storage words of the packed formats, host and device: a 64-bit torus word leaves the keyswitch arithmetic as its
// closest 32-bit word (string store, compact strings) or 16-bit word (packed download), ties upwards, the carry out of
// the top dropped.  Every kernel and every host reference that stores such a word rounds it here.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define FHS_HOST_DEVICE __host__ __device__
#else
#define FHS_HOST_DEVICE
#endif

namespace fhs {

FHS_HOST_DEVICE inline uint32_t round32(uint64_t x) { return (uint32_t)((x + (1ull << 31)) >> 32); }
FHS_HOST_DEVICE inline uint16_t round16(uint64_t x) { return (uint16_t)((x + (1ull << 47)) >> 48); }
// round16((uint64_t)w << 32) in its 32-bit form: the same word (the sum wraps to 0 where the 64-bit one carries out of
// the top), kept so that the streaming kernel of store_kernels.hip compiles to the code it had.
FHS_HOST_DEVICE inline uint16_t store_round16(uint32_t w) { return (uint16_t)((w + (1u << 15)) >> 16); }

// The launchers' range check: `groups` groups of `group` words hold `total` words when the last group is not empty,
// ceil(total / group) == groups.
inline bool fills_groups(size_t total, int groups, size_t group) {
    return groups > 0 && total > (size_t)(groups - 1) * group && total <= (size_t)groups * group;
}

}  // namespace fhs
