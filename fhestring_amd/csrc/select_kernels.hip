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
// blockIdx.y is the query of a batched call (fhs_store_select_batch).  Below it, select_query_to_ntt_kernel: the query
// from torus words, or from a seed and bodies, to the transform domain.
#include "../../include/fhestring_hip.h"
#include "chacha_device.h"
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
    // query blockIdx.y of the call: its own source (stride 0 while every query still reads the entry), destination and
    // GGSWs.  All of it is uniform over the workgroup, so the offsets stay in scalar registers.
    const size_t src_off = (size_t)blockIdx.y * P.src_stride, dst_off = (size_t)blockIdx.y * P.dst_stride;
    const double *query_ntt = P.query_ntt + (size_t)blockIdx.y * P.query_stride;
    const uint32_t *a_mask = P.src_mask + src_off + (size_t)na * POLY_N, *a_body = P.src_body + src_off + (size_t)na * SELECT_GROUP;
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
        query_ntt, P.bit, ks);

    // the last launch (one node) writes into the new entries themselves: mask[2048] | body, one allocation per query
    const uint32_t node = blockIdx.x;
    uint32_t *dst_mask = P.dst_table ? P.dst_table[blockIdx.y] : P.dst_mask + dst_off;
    uint32_t *dst_body = P.dst_table ? dst_mask + POLY_N : P.dst_body + dst_off;
    if (j == 0) {
        uint32_t *out = dst_mask + (size_t)node * POLY_N;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            out[n] = round32(((uint64_t)a_mask[n] << 32) + ks[o]);
        }
    } else {
        uint32_t *out = dst_body + (size_t)node * SELECT_GROUP;
#pragma unroll
        for (int o = 0; o < 16; o++) {
            const uint32_t n = lane + 64 * (2 * o + q);
            if (n < P.store_body) out[n] = round32(((uint64_t)(n < a_count ? a_body[n] : 0u) << 32) + ks[o]);
        }
    }
}

// ---- the query to the transform domain ----------------------------------------------------------------------------------
// One wavefront per (polynomial, prime), four per workgroup, each with one transform region of LDS as in
// glwe_keyswitch.h.  A polynomial is 2048 torus words from memory or, the mask of a seeded row, 2048 draws of its
// ChaCha20 stream: a block yields 8 CONSECUTIVE draws while the transform wants coefficient lane + 64 r, so the wave
// makes its 256 blocks cooperatively, four per lane, into its LDS region and reads them back strided; the draws never
// reach memory.  The doubles written equal convert_polys_to_ntt's (ntt_tables.cpp) bit for bit:
//   1. v = (int64)round_to_grid(w, quant_bits) >> quant_bits, in wrapping 64-bit integers as on the host, |v| <= 2^63 >>
//      quant_bits.  With p = 2^47 - c (c < 2^17): v = hi 2^47 + lo, hi = v >> 47 (|hi| <= 2^16), 0 <= lo < 2^47, so
//      v = lo + hi c (mod p), an integer in (-2^33, 2^47 + 2^33); above (p - 1) / 2 it loses p once: |x| <= (p - 1) / 2.
//   2. ntt_forward, unchanged.  EXACTNESS.  The keyswitch kernels feed it digits below 2^15; here the inputs are full
//      residues, |x| <= p / 2.  Every one of the eleven stages is x +- v with v = mulmod(., w): |v| <= p (1/2 + |a| 2^-53)
//      <= p (1/2 + m / 64) for an input of magnitude m p (p < 2^47).  Nothing is reduced in between, so m_0 = 1/2 and
//      m_(k+1) = m_k + 1/2 + m_k / 64: m_11 = 6.55 (bounded by 1/2 + 11 x 0.6 = 7.1).  7.1 p < 2^50: every value is an
//      integer below the 2^52 that mulmod is exact for, and no reduce_once is needed.
//   3. mulmod by N^-1 = -(p - 1) / 2048 (mod p): |r| <= p (1/2 + 7.1 / 64) < p, congruent to the host's residue.
//   4. The host stores centred(): the representative in [-(p - 1) / 2, (p - 1) / 2].  One conditional -+ p gets there
//      from |r| < p, and + 0.0 turns a negative zero into the host's +0.0.
// General in the number of polynomials and in quant_bits: the key loads may adopt it.
__global__ __launch_bounds__(256) void select_query_to_ntt_kernel(SelectQueryParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t g = blockIdx.x * 4 + wave, poly = g >> 1;       // g & 1 == wave & 1: the prime, as KeyswitchWave takes it
    if (poly >= P.n_polys) return;                                 // whole waves; the kernel has no workgroup barrier
    const KeyswitchWave w(P.tw, smem, lane, wave);
    const uint64_t grid = ~(((uint64_t)1 << P.quant_bits) - 1), half = (uint64_t)1 << (P.quant_bits - 1);

    uint64_t t[32];                                                // t[r] = torus word of coefficient lane + 64 r
    const uint32_t qi = P.seeds ? poly / P.query_polys : 0u, in_query = P.seeds ? poly % P.query_polys : 0u;
    if (P.seeds && !(in_query & 1)) {                              // the mask of GGSW row in_query / 2 of seeded query qi
        SeedKey seed;
#pragma unroll
        for (int i = 0; i < 8; i++) seed.w[i] = P.seeds[(size_t)qi * 8 + i];
        uint64_t *stage = reinterpret_cast<uint64_t *>(w.my);      // 2048 of the region's 2176 slots
#pragma unroll 1
        for (int i = 0; i < 4; i++) {
            const uint32_t blk = lane + 64 * i;
            uint64_t d[8];
            chacha20_block(seed, blk, FHS_DOM_SEEDED_SELECT, in_query >> 1, 0u, d);
            ulonglong2 *l = reinterpret_cast<ulonglong2 *>(stage + 8 * blk);
#pragma unroll
            for (int k = 0; k < 4; k++) l[k] = make_ulonglong2(d[2 * k], d[2 * k + 1]);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 32; r++) t[r] = stage[lane + 64 * r] & grid;
        __builtin_amdgcn_wave_barrier();                           // ... before the transform writes the region
    } else {
        // full form: polynomial `poly` of the words; seeded: the body of row in_query / 2 among the query's bodies
        const size_t at = P.seeds ? (size_t)qi * (P.query_polys >> 1) + (in_query >> 1) : (size_t)poly;
        const uint64_t *src = P.words + at * POLY_N;
#pragma unroll
        for (int r = 0; r < 32; r++) t[r] = src[lane + 64 * r];
    }

    const int64_t pi = w.q ? (int64_t)NTT_P1 : (int64_t)NTT_P0, c = ((int64_t)1 << 47) - pi;
    double x[32];
#pragma unroll
    for (int r = 0; r < 32; r++) {
        const int64_t v = (int64_t)((t[r] + half) & grid) >> P.quant_bits;
        int64_t m = (v & (((int64_t)1 << 47) - 1)) + (v >> 47) * c;
        if (m > (pi - 1) / 2) m -= pi;
        x[r] = (double)m;
    }
    ntt_forward(x, w.my, lane, w.twA, w.fwd_lane, w.p, w.pinv);

    typedef double __attribute__((ext_vector_type(2))) double2_t;
    const double ninv = -(double)((pi - 1) / POLY_N), bound = (double)((pi - 1) / 2);
    double2_t *out = reinterpret_cast<double2_t *>(P.out + ((size_t)poly * 2 + w.q) * POLY_N) + lane;
#pragma unroll
    for (int cc = 0; cc < 32; cc += 2) {
        double o[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const double r = mulmod(x[cc + h], ninv, w.p, w.pinv);
            o[h] = (r > bound ? r - w.p : (r < -bound ? r + w.p : r)) + 0.0;
        }
        out[(cc >> 1) * 64] = double2_t{o[0], o[1]};               // [16][64 lanes][2]: slots (cc, cc + 1) of this lane
    }
}

hipError_t prepare_device_for_select() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(select_cmux_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)keyswitch_lds_bytes());
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(select_query_to_ntt_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)keyswitch_lds_bytes());
}

hipError_t launch_select_query_to_ntt(const SelectQueryParams &p, hipStream_t s) {
    if (!p.words || !p.out || p.n_polys == 0 || p.n_polys > (1u << 24) || p.quant_bits < 1 || p.quant_bits > 32)
        return hipErrorInvalidValue;
    if (p.seeds && (p.query_polys == 0 || (p.query_polys & 1) || p.n_polys % p.query_polys)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_query_to_ntt_kernel, dim3((p.n_polys + 1) / 2), dim3(256), keyswitch_lds_bytes(), s, p);
    return hipGetLastError();
}

hipError_t launch_select_cmux(const SelectCmuxParams &p, hipStream_t s) {
    if (!p.src_mask || !p.src_body || !p.query_ntt || p.bit < 0 || p.queries == 0 || p.queries > 65535u) return hipErrorInvalidValue;
    if (!p.dst_table && (!p.dst_mask || !p.dst_body)) return hipErrorInvalidValue;
    if (p.src_nodes == 0 || !fills_groups(p.src_body_total, (int)p.src_nodes, SELECT_GROUP)) return hipErrorInvalidValue;
    if (p.rotate >= (uint32_t)POLY_N || p.store_body == 0 || p.store_body > (uint32_t)SELECT_GROUP) return hipErrorInvalidValue;
    if (p.src_mask == p.dst_mask || p.src_body == p.dst_body) return hipErrorInvalidValue;       // never in place
    const uint32_t grid = p.rotate ? p.src_nodes : (p.src_nodes + 1) / 2;
    if (p.dst_table && grid != 1) return hipErrorInvalidValue;                                   // an entry is one node
    hipLaunchKernelGGL(select_cmux_kernel, dim3(grid, p.queries), dim3(256), keyswitch_lds_bytes(), s, p);
    return hipGetLastError();
}

}  // namespace fhs
