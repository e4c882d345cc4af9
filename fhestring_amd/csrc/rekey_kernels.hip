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
// keyswitch_sums.
#include "ntt_transform.h"
#include "rekey_kernels.h"

namespace fhs {

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ uint32_t switch32(uint64_t x) { return (uint32_t)((x + (1ull << 31)) >> 32); }
__device__ __forceinline__ uint16_t switch16(uint64_t x) { return (uint16_t)((x + (1ull << 47)) >> 48); }
static_assert(REKEY_LEVELS == 2 && REKEY_BASE_LOG == 16, "the digits are the two 16-bit halves of a 32-bit word");

// The keyswitch between load and store, shared by all three kernels: from the group's mask as 32-bit words in the strided
// layout (a[r] = word of coefficient lane + 64 r) to ks[o] = (sum_l d_l (*) K[l][j]) of coefficient lane + 64 (2 o + q),
// the half of output polynomial j that wave (j, q) owns.  Holds the workgroup's one barrier: every wave's loads of `a`
// are behind it when it returns, so the caller may store over its source.
__device__ __forceinline__ void keyswitch_sums(const uint32_t (&a)[32], const double *key_ntt, const NttTables &tw, char *smem,
                                               int lane, int wave, uint64_t (&ks)[16]) {
    const int j = wave >> 1;   // output polynomial (0 mask, 1 body)
    const int q = wave & 1;    // prime
    double *my = reinterpret_cast<double *>(smem) + wave * LDS_WAVE_SLOTS;
    const double *sibling = reinterpret_cast<double *>(smem) + (wave ^ 1) * LDS_WAVE_SLOTS;  // other prime
    uint64_t *my_u = reinterpret_cast<uint64_t *>(my);

    const double p = q ? (double)NTT_P1 : (double)NTT_P0;
    const double pinv = 1.0 / p;
    const double p1 = (double)NTT_P1, p1inv = 1.0 / p1;
    const double *fwd_lane = tw.fwd_lane + q * 32 * 64;
    const double *inv_lane = tw.inv_lane + q * 32 * 64;
    const double twA = lane < 32 ? C_FWD_UNI[q][lane] : C_INV_UNI[q][lane];
    const double twB = C_INV_UNI[q][lane & 31];

    // sum over the digits of NTT(d_l) * NTT(K[l][j]) modulo p
    typedef double __attribute__((ext_vector_type(2))) double2_t;
    double acc[32];
#pragma unroll
    for (int c = 0; c < 32; c++) acc[c] = 0.0;
#pragma unroll
    for (int l = 0; l < REKEY_LEVELS; l++) {
        double x[32];
#pragma unroll
        for (int r = 0; r < 32; r++) {
            const uint32_t lo = a[r] & 0xffffu;
            // l = 1: the low half as a signed 16-bit value; l = 0: the high half plus the carry of a negative low digit
            x[r] = l ? (double)(int16_t)(uint16_t)lo : (double)(int16_t)(uint16_t)((a[r] >> 16) + (lo >= 0x8000u ? 1u : 0u));
        }
        __builtin_amdgcn_wave_barrier();
        ntt_forward(x, my, lane, twA, fwd_lane, p, pinv);
        // key layout [16][64 lanes][2]: one 16-byte load per lane covers coefficients (c, c + 1) of the contiguous layout
        const double2_t *key = reinterpret_cast<const double2_t *>(key_ntt + ((((size_t)l * 2 + j) * 2 + q) * POLY_N)) + lane;
#pragma unroll
        for (int c = 0; c < 32; c += 2) {
            const double2_t kv = key[(c >> 1) * 64];
            const double m0 = mulmod(x[c], kv.x, p, pinv), m1 = mulmod(x[c + 1], kv.y, p, pinv);
            acc[c] += m0;
            acc[c + 1] += m1;
        }
    }
#pragma unroll
    for (int c = 0; c < 32; c++) acc[c] = reduce_once(acc[c], p, pinv);   // two products: back inside the inverse's input range
    __builtin_amdgcn_wave_barrier();
    ntt_inverse(acc, my, lane, twA, twB, inv_lane, p, pinv);
    __builtin_amdgcn_wave_barrier();

    // exchange residues with the other prime's wave, CRT for the owned half (coefficients lane + 64 (2 o + q))
#pragma unroll
    for (int o = 0; o < 16; o++) ks[o] = 0;
    if (q == 0) phase_publish_residues<0>(acc, my, lane);
    else phase_publish_residues<1>(acc, my, lane);
    __syncthreads();                                  // ... and every wave's mask loads are behind it: stores may begin
    if (q == 0) phase_crt<0>(acc, ks, sibling, my_u, lane, C_CRT, p1, p1inv);
    else phase_crt<1>(acc, ks, sibling, my_u, lane, C_CRT, p1, p1inv);
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
        for (int o = 0; o < 16; o++) out[lane + 64 * (2 * o + q)] = switch32((uint64_t)0 - ks[o]);
    } else {
        const uint32_t *in = P.src_body + (size_t)grp * REKEY_GROUP;
        uint32_t *out = P.dst_body + (size_t)grp * REKEY_GROUP;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            if (n < count) out[n] = switch32(((uint64_t)in[n] << 32) - ks[o]);
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
    for (int r = 0; r < 32; r++) a[r] = switch32(src_mask[lane + 64 * r]);

    uint64_t ks[16];
    keyswitch_sums(a, P.key_ntt, P.tw, smem, lane, wave, ks);

    if (j == 0) {
        uint16_t *out = P.dst_mask + (size_t)grp * POLY_N;
#pragma unroll
        for (int o = 0; o < 16; o++) out[lane + 64 * (2 * o + q)] = switch16((uint64_t)0 - ks[o]);
    } else {
        uint16_t *out = P.dst_body + (size_t)grp * REKEY_GROUP;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            if (n < count) out[n] = switch16(src_body[n] - ks[o]);
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
        for (int o = 0; o < 16; o++) out[lane + 64 * (2 * o + q)] = switch16((uint64_t)0 - ks[o]);
    } else {
        const uint32_t *in = P.src_body + (size_t)base;
        uint16_t *out = P.dst_body;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            if (lo <= n && n < hi) out[base + n - P.first_coef] = switch16(((uint64_t)in[n] << 32) - ks[o]);
        }
    }
}

static size_t rekey_lds_bytes() { return (size_t)4 * LDS_WAVE_SLOTS * sizeof(double); }

hipError_t prepare_device_for_rekey() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(rekey_glwe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)rekey_lds_bytes());
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(rekey_packed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)rekey_lds_bytes());
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(rekey_entry_packed_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)rekey_lds_bytes());
}

hipError_t launch_rekey_glwe(const RekeyParams &p, hipStream_t s) {
    if (p.groups <= 0 || p.total == 0 || !p.src_mask || !p.src_body || !p.dst_mask || !p.dst_body || !p.key_ntt)
        return hipErrorInvalidValue;
    if ((size_t)p.total > (size_t)p.groups * REKEY_GROUP || (size_t)p.total <= (size_t)(p.groups - 1) * REKEY_GROUP)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rekey_glwe_kernel, dim3(p.groups), dim3(256), rekey_lds_bytes(), s, p);
    return hipGetLastError();
}

hipError_t launch_rekey_packed(const RekeyPackedParams &p, hipStream_t s) {
    if (p.groups <= 0 || p.total == 0 || !p.src || !p.dst_mask || !p.dst_body || !p.key_ntt) return hipErrorInvalidValue;
    if ((size_t)p.total > (size_t)p.groups * REKEY_GROUP || (size_t)p.total <= (size_t)(p.groups - 1) * REKEY_GROUP)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rekey_packed_kernel, dim3(p.groups), dim3(256), rekey_lds_bytes(), s, p);
    return hipGetLastError();
}

hipError_t launch_rekey_entry_packed(const RekeyEntryPackedParams &p, hipStream_t s) {
    if (p.groups <= 0 || p.body_words == 0 || !p.src_mask || !p.src_body || !p.dst_mask || !p.dst_body || !p.key_ntt)
        return hipErrorInvalidValue;
    const size_t end = (size_t)p.first_coef + p.body_words;          // the last covering group holds its last coefficient
    if (p.first_coef >= (uint32_t)REKEY_GROUP || end > (size_t)p.groups * REKEY_GROUP || end <= (size_t)(p.groups - 1) * REKEY_GROUP)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rekey_entry_packed_kernel, dim3(p.groups), dim3(256), rekey_lds_bytes(), s, p);
    return hipGetLastError();
}

}  // namespace fhs
