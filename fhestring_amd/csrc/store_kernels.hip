// Device-resident string store on gfx950 (include/fhestring_hip.h, "device-resident string store").
// A parked string is the output of the ring-packing tree (pack_kernels.hip) with every word rounded to 32 bits,
// (x + 2^31) >> 32 -- word for word the compact-string format of the public-key uploads, so expand_public_blocks_kernel
// (pk_kernels.hip) brings it back.  The only kernel the store adds is this switch: it reads the level-11 GLWEs where the
// tree left them and writes the 32-bit words straight into the entry's own allocation (no intermediate buffer, nothing
// crosses the bus).  Pure streaming: every lane loads two consecutive u64 (16 bytes) and stores two u32 (8 bytes), a
// wavefront reads 1 KiB and writes 512 B contiguous; no LDS, no scratch.  Not part of any bootstrap.
// store_switch16_kernel is the way out under the entry's own key: a window of a parked entry leaves
// as the packed download's 16-bit words without being expanded -- the masks of the covering groups and the window's bodies,
// every word (w + 2^15) >> 16.  Mask words come in whole groups and bodies four to a character, so every lane takes
// exactly four words: one 16-byte load, one 8-byte store, and no lane has a tail.
#include <hip/hip_runtime.h>

#include "pack_kernels.h"
#include "storage_words.h"
#include "store_kernels.h"

namespace fhs {

namespace {

typedef uint64_t __attribute__((ext_vector_type(2))) u64x2_t;

// grid (8, groups): workgroups 0..3 of a group switch the four quarters of its mask, 4..7 those of its body, of which only
// the words of present blocks are written (the entry holds no others).
__global__ __launch_bounds__(256) void store_switch32_kernel(const uint64_t *__restrict__ glwe, uint32_t *__restrict__ mask32,
                                                             uint32_t *__restrict__ body32, uint32_t first_group,
                                                             uint32_t total) {
    const uint32_t grp = blockIdx.y, col = blockIdx.x >> 2;
    const uint32_t w = 2 * ((blockIdx.x & 3) * 256 + threadIdx.x);          // the first of this lane's two words
    const uint32_t count = col ? min((uint32_t)PACK_GROUP, total - grp * PACK_GROUP) : (uint32_t)POLY_N;
    if (w >= count) return;
    const u64x2_t v = *reinterpret_cast<const u64x2_t *>(glwe + ((size_t)grp * 2 + col) * POLY_N + w);
    // group first_group + grp of the ENTRY: masks and bodies both advance by 2048 words per group
    uint32_t *dst = (col ? body32 : mask32) + (size_t)(first_group + grp) * POLY_N + w;
    if (w + 1 < count) *reinterpret_cast<uint2 *>(dst) = make_uint2(round32(v.x), round32(v.y));
    else *dst = round32(v.x);                                          // an odd block count's last body
}

// One launch over both arrays: quads [0, mask_quads) are the covering groups' masks, [mask_quads, mask_quads + body_quads)
// the window's bodies (body32 points at the window's first body inside the entry, body16 at output word 0).
__global__ __launch_bounds__(256) void store_switch16_kernel(const uint32_t *__restrict__ mask32, const uint32_t *__restrict__ body32,
                                                             uint16_t *__restrict__ mask16, uint16_t *__restrict__ body16,
                                                             uint32_t mask_quads, uint32_t body_quads) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t *src = mask32;
    uint16_t *dst = mask16;
    if (i >= mask_quads) {
        i -= mask_quads;
        if (i >= body_quads) return;
        src = body32;
        dst = body16;
    }
    const uint4 v = *reinterpret_cast<const uint4 *>(src + 4 * (size_t)i);
    *reinterpret_cast<ushort4 *>(dst + 4 * (size_t)i) =
        make_ushort4(store_round16(v.x), store_round16(v.y), store_round16(v.z), store_round16(v.w));
}

}  // namespace

hipError_t launch_store_switch16(const uint32_t *mask32, const uint32_t *body32, uint16_t *mask16, uint16_t *body16, int groups,
                                 size_t body_words, hipStream_t s) {
    if (groups <= 0 || body_words == 0 || (body_words & 3) || body_words > (size_t)groups * PACK_GROUP) return hipErrorInvalidValue;
    if (((uintptr_t)mask32 & 15) || ((uintptr_t)body32 & 15) || ((uintptr_t)mask16 & 7) || ((uintptr_t)body16 & 7))
        return hipErrorInvalidValue;
    const uint32_t mask_quads = (uint32_t)groups * (POLY_N / 4), body_quads = (uint32_t)(body_words / 4);
    hipLaunchKernelGGL(store_switch16_kernel, dim3((mask_quads + body_quads + 255) / 256), dim3(256), 0, s, mask32, body32, mask16,
                       body16, mask_quads, body_quads);
    return hipGetLastError();
}

hipError_t launch_store_switch32(const uint64_t *d_glwe, uint32_t *entry_mask32, uint32_t *entry_body32,
                                 uint32_t first_group, int groups, uint32_t total, hipStream_t s) {
    if (!fills_groups(total, groups, PACK_GROUP)) return hipErrorInvalidValue;
    if (((uintptr_t)d_glwe & 15) || ((uintptr_t)entry_mask32 & 7) || ((uintptr_t)entry_body32 & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(store_switch32_kernel, dim3(8, groups), dim3(256), 0, s, d_glwe, entry_mask32, entry_body32, first_group,
                       total);
    return hipGetLastError();
}

}  // namespace fhs
