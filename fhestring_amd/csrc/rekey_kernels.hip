// Re-key of string-store entries on gfx950: one GLWE keyswitch per group of 2048 blocks from the client key S_old the
// entry is under to S_new, with the exact two-prime NTT of the blind rotation (ntt_transform.h).  DESIGN.md section 14;
// host reference with the same words: rekey_host.cpp.
//
// One workgroup (4 wavefronts) per group.  With A = mask32 << 32 = d_0 2^48 + d_1 2^32 (balanced 16-bit digits: a stored
// word has 32 significant bits, so the decomposition is exact),
//     mask' = -sum_l d_l (*) K[l].mask,   body'_j = (body32_j << 32) - (sum_l d_l (*) K[l].body)_j  for j < count,
// every word stored as (x + 2^31) >> 32.  Wavefront (j, q) owns output polynomial j (0 mask, 1 body) modulo prime q, as
// in pack_level_kernel and blind_rotate_kernel; every wave reads the whole mask (256 B contiguous per wave instruction)
// and transforms both digit polynomials under its prime.
// In place: every wave has read the whole mask before the workgroup barrier and every store comes after it; a body word is
// read and written by the same lane; groups touch disjoint words.  So dst may be src.
// rekey_packed_kernel is the same keyswitch between other formats: 64-bit words in, 16-bit words out (DESIGN.md section
// 16; host reference fhs_rekey_packed_host), and rekey_entry_packed_kernel takes a window of a parked entry, 32-bit words,
// to 16-bit words (section 17; fhs_store_packed_host).  The arithmetic between load and store exists once, in
// glwe_keyswitch_sums (glwe_keyswitch.h), which the packing tree calls too.
#include "glwe_keyswitch.h"
#include "rekey_kernels.h"
#include "storage_words.h"

namespace fhs {

#pragma clang fp contract(off)

namespace {

static_assert(REKEY_LEVELS == 2 && REKEY_BASE_LOG == 16, "the digits are the two 16-bit halves of a 32-bit word");

// The keyswitch between load and store, shared by all three kernels (glwe_keyswitch.h): from the group's mask as 32-bit
// words in the strided layout (a[r] = word of coefficient lane + 64 r) to ks[o] of coefficient lane + 64 (2 o + q).
__device__ __forceinline__ void keyswitch_sums(const uint32_t (&a)[32], const double *key_ntt, const NttTables &tw, char *smem,
                                               int lane, int wave, uint64_t (&ks)[16]) {
    glwe_keyswitch_sums<REKEY_LEVELS>(
        KeyswitchWave(tw, smem, lane, wave),
        [a](int r, int l) {
            const uint32_t lo = a[r] & 0xffffu;
            // l = 1: the low half as a signed 16-bit value; l = 0: the high half plus the carry of a negative low digit
            return l ? (double)(int16_t)(uint16_t)lo : (double)(int16_t)(uint16_t)((a[r] >> 16) + (lo >= 0x8000u ? 1u : 0u));
        },
        key_ntt, 0, ks);
}

}  // namespace

__global__ __launch_bounds__(256) void rekey_glwe_kernel(RekeyParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t grp = blockIdx.x;
    const uint32_t count = min((uint32_t)REKEY_GROUP, P.total - grp * REKEY_GROUP);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = wave >> 1, q = wave & 1;

    // the group's mask, strided layout: a[r] = word of coefficient lane + 64 r
    const uint32_t *src_mask = P.src_mask + (size_t)grp * POLY_N;
    uint32_t a[32];
#pragma unroll
    for (int r = 0; r < 32; r++) a[r] = src_mask[lane + 64 * r];

    uint64_t ks[16];
    keyswitch_sums(a, P.key_ntt, P.tw, smem, lane, wave, ks);

    if (j == 0) {
        uint32_t *out = P.dst_mask + (size_t)grp * POLY_N;
#pragma unroll
        for (int o = 0; o < 16; o++) out[lane + 64 * (2 * o + q)] = round32((uint64_t)0 - ks[o]);
    } else {
        const uint32_t *in = P.src_body + (size_t)grp * REKEY_GROUP;
        uint32_t *out = P.dst_body + (size_t)grp * REKEY_GROUP;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            if (n < count) out[n] = round32(((uint64_t)in[n] << 32) - ks[o]);
        }
    }
}

// The packed download for a recipient: the same keyswitch from the packing tree's level-11 GLWE,
// 64-bit words (mask[2048] | body[2048] per group), to 16-bit words under S_new.  The mask is rounded to 32 bits in
// registers as it is loaded (512 B contiguous per wave instruction); the body keeps its 64 bits and is read after the
// barrier by the lane that stores it; one rounding, to 16 bits, at the end.  Source and destination are different buffers.
__global__ __launch_bounds__(256) void rekey_packed_kernel(RekeyPackedParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t grp = blockIdx.x;
    const uint32_t count = min((uint32_t)REKEY_GROUP, P.total - grp * REKEY_GROUP);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = wave >> 1, q = wave & 1;

    const uint64_t *src_mask = P.src + (size_t)grp * 2 * POLY_N, *src_body = src_mask + POLY_N;
    uint32_t a[32];
#pragma unroll
    for (int r = 0; r < 32; r++) a[r] = round32(src_mask[lane + 64 * r]);

    uint64_t ks[16];
    keyswitch_sums(a, P.key_ntt, P.tw, smem, lane, wave, ks);

    if (j == 0) {
        uint16_t *out = P.dst_mask + (size_t)grp * POLY_N;
#pragma unroll
        for (int o = 0; o < 16; o++) out[lane + 64 * (2 * o + q)] = round16((uint64_t)0 - ks[o]);
    } else {
        uint16_t *out = P.dst_body + (size_t)grp * REKEY_GROUP;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            if (n < count) out[n] = round16(src_body[n] - ks[o]);
        }
    }
}

// The packed download of a parked entry for a recipient: the mask is loaded as rekey_glwe_kernel
// loads it (the stored word has 32 significant bits: nothing is rounded on the way in), the words are stored as
// rekey_packed_kernel stores them.  Workgroup g takes covering group g of the window; only the window's coefficients of
// that group have a body -- [lo, hi) is partial in the first and the last covering group -- and a body word is read after
// the barrier by the lane that stores it.  Source (the entry) and destination are different buffers; the entry is only read.
__global__ __launch_bounds__(256) void rekey_entry_packed_kernel(RekeyEntryPackedParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t grp = blockIdx.x;
    // the window's coefficient range inside this group (the launcher checked that the last group holds `end - 1`)
    const uint32_t base = grp * REKEY_GROUP, end = P.first_coef + P.body_words;
    const uint32_t lo = P.first_coef > base ? P.first_coef - base : 0u;
    const uint32_t hi = min((uint32_t)REKEY_GROUP, end - base);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = wave >> 1, q = wave & 1;

    const uint32_t *src_mask = P.src_mask + (size_t)grp * POLY_N;
    uint32_t a[32];
#pragma unroll
    for (int r = 0; r < 32; r++) a[r] = src_mask[lane + 64 * r];

    uint64_t ks[16];
    keyswitch_sums(a, P.key_ntt, P.tw, smem, lane, wave, ks);

    if (j == 0) {
        uint16_t *out = P.dst_mask + (size_t)grp * POLY_N;
#pragma unroll
        for (int o = 0; o < 16; o++) out[lane + 64 * (2 * o + q)] = round16((uint64_t)0 - ks[o]);
    } else {
        const uint32_t *in = P.src_body + (size_t)base;
        uint16_t *out = P.dst_body;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            if (lo <= n && n < hi) out[base + n - P.first_coef] = round16(((uint64_t)in[n] << 32) - ks[o]);
        }
    }
}

hipError_t prepare_device_for_rekey() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(rekey_glwe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)keyswitch_lds_bytes());
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(rekey_packed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)keyswitch_lds_bytes());
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(rekey_entry_packed_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)keyswitch_lds_bytes());
}

hipError_t launch_rekey_glwe(const RekeyParams &p, hipStream_t s) {
    if (p.groups <= 0 || p.total == 0 || !p.src_mask || !p.src_body || !p.dst_mask || !p.dst_body || !p.key_ntt)
        return hipErrorInvalidValue;
    if (!fills_groups(p.total, p.groups, REKEY_GROUP)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rekey_glwe_kernel, dim3(p.groups), dim3(256), keyswitch_lds_bytes(), s, p);
    return hipGetLastError();
}

hipError_t launch_rekey_packed(const RekeyPackedParams &p, hipStream_t s) {
    if (p.groups <= 0 || p.total == 0 || !p.src || !p.dst_mask || !p.dst_body || !p.key_ntt) return hipErrorInvalidValue;
    if (!fills_groups(p.total, p.groups, REKEY_GROUP)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rekey_packed_kernel, dim3(p.groups), dim3(256), keyswitch_lds_bytes(), s, p);
    return hipGetLastError();
}

hipError_t launch_rekey_entry_packed(const RekeyEntryPackedParams &p, hipStream_t s) {
    if (p.groups <= 0 || p.body_words == 0 || !p.src_mask || !p.src_body || !p.dst_mask || !p.dst_body || !p.key_ntt)
        return hipErrorInvalidValue;
    const size_t end = (size_t)p.first_coef + p.body_words;          // the last covering group holds its last coefficient
    if (p.first_coef >= (uint32_t)REKEY_GROUP || !fills_groups(end, p.groups, REKEY_GROUP)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rekey_entry_packed_kernel, dim3(p.groups), dim3(256), keyswitch_lds_bytes(), s, p);
    return hipGetLastError();
}

}  // namespace fhs
