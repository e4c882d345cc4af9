// Select by encrypted index on string-store entries, gfx950: one CMux per workgroup (4 wavefronts), the external product
// of the difference of two 32-bit GLWEs with the GGSW of one index bit, on the exact two-prime NTT of the blind rotation
// (ntt_transform.h).  DESIGN.md section 23; host reference with the same words: select_host.cpp.
//
// With D = (b - a) mod 2^32 word by word, mask and body, and D << 32 = d_0 2^48 + d_1 2^32 (balanced 16-bit digits, exact
// as in rekey_kernels.hip), the four digit polynomials (mask d_0, mask d_1, body d_0, body d_1) meet the four rows of the
// bit's GGSW:
//     out_col = round32((a_col << 32) + sum_l d_l (*) GGSW[l].col)     for col = mask, body.
// That sum is glwe_keyswitch_sums with four digits instead of the re-key's two, the GGSW of bit k as key set k.  Wavefront
// (j, q) owns output polynomial j (0 mask, 1 body) modulo prime q; every wave reads both operands whole (256 B contiguous
// per wave instruction) and keeps the two differences in registers, 64 words, through the four forward transforms.
// NOT in place: workgroup i writes node i of the destination while others read nodes 2i and 2i + 1 of the source, so the
// launcher's buffers alternate.  The words of `a` are read again after the barrier by the lane that stores them.
#include "glwe_keyswitch.h"
#include "select_kernels.h"
#include "storage_words.h"

namespace fhs {

#pragma clang fp contract(off)

namespace {

// digit l & 1 of a 32-bit word as rekey_kernels.hip takes them: 1 = the low half as a signed 16-bit value, 0 = the high
// half plus the carry of a negative low digit
__device__ __forceinline__ double digit16(uint32_t w, int low) {
    const uint32_t lo = w & 0xffffu;
    return low ? (double)(int16_t)(uint16_t)lo : (double)(int16_t)(uint16_t)((w >> 16) + (lo >= 0x8000u ? 1u : 0u));
}

}  // namespace

__global__ __launch_bounds__(256) void select_cmux_kernel(SelectCmuxParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = wave >> 1, q = wave & 1;
    const uint32_t s = P.rotate;
    const uint32_t na = s ? blockIdx.x : 2 * blockIdx.x, nb = na + 1;            // na < src_nodes (the launcher's grid)
    const uint32_t *a_mask = P.src_mask + (size_t)na * POLY_N, *a_body = P.src_body + (size_t)na * SELECT_GROUP;
    const uint32_t a_count = min((uint32_t)SELECT_GROUP, P.src_body_total - na * SELECT_GROUP);
    const bool has_b = !s && nb < P.src_nodes;                                   // otherwise the zero GLWE, or X^-s a
    const uint32_t *b_mask = a_mask + POLY_N, *b_body = a_body + SELECT_GROUP;   // read only where has_b
    const uint32_t b_count = has_b ? min((uint32_t)SELECT_GROUP, P.src_body_total - nb * SELECT_GROUP) : 0u;

    // D = b - a in the strided layout: dm[r], db[r] = mask and body word of coefficient lane + 64 r
    uint32_t dm[32], db[32];
#pragma unroll
    for (int r = 0; r < 32; r++) {
        const uint32_t n = lane + 64 * r;
        const uint32_t am = a_mask[n], ab = n < a_count ? a_body[n] : 0u;
        uint32_t bm = 0u, bb = 0u;
        if (s) {                                             // (X^-s a)_n = a_(n + s), negated where it wraps
            const uint32_t m = (n + s) & (POLY_N - 1);
            bm = a_mask[m];
            bb = m < a_count ? a_body[m] : 0u;
            if (n + s >= (uint32_t)POLY_N) { bm = 0u - bm; bb = 0u - bb; }
        } else if (has_b) {
            bm = b_mask[n];
            bb = n < b_count ? b_body[n] : 0u;
        }
        dm[r] = bm - am;
        db[r] = bb - ab;
    }

    uint64_t ks[16];
    glwe_keyswitch_sums<SELECT_DIGITS>(
        KeyswitchWave(P.tw, smem, lane, wave),
        [dm, db](int r, int l) { return digit16(l < 2 ? dm[r] : db[r], l & 1); },
        P.query_ntt, P.bit, ks);

    const uint32_t node = blockIdx.x;
    if (j == 0) {
        uint32_t *out = P.dst_mask + (size_t)node * POLY_N;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            out[n] = round32(((uint64_t)a_mask[n] << 32) + ks[o]);
        }
    } else {
        uint32_t *out = P.dst_body + (size_t)node * SELECT_GROUP;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            if (n < P.store_body) out[n] = round32(((uint64_t)(n < a_count ? a_body[n] : 0u) << 32) + ks[o]);
        }
    }
}

hipError_t prepare_device_for_select() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(select_cmux_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)keyswitch_lds_bytes());
}

hipError_t launch_select_cmux(const SelectCmuxParams &p, hipStream_t s) {
    if (!p.src_mask || !p.src_body || !p.dst_mask || !p.dst_body || !p.query_ntt || p.bit < 0) return hipErrorInvalidValue;
    if (p.src_nodes == 0 || !fills_groups(p.src_body_total, (int)p.src_nodes, SELECT_GROUP)) return hipErrorInvalidValue;
    if (p.rotate >= (uint32_t)POLY_N || p.store_body == 0 || p.store_body > (uint32_t)SELECT_GROUP) return hipErrorInvalidValue;
    if (p.src_mask == p.dst_mask || p.src_body == p.dst_body) return hipErrorInvalidValue;       // never in place
    const uint32_t grid = p.rotate ? p.src_nodes : (p.src_nodes + 1) / 2;
    hipLaunchKernelGGL(select_cmux_kernel, dim3(grid), dim3(256), keyswitch_lds_bytes(), s, p);
    return hipGetLastError();
}

}  // namespace fhs
