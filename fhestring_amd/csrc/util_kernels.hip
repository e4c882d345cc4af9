// Small data-movement kernels that are not part of any bootstrap (kept out of the profiled kernel sources:
// fhestring_amd/kernel_sources.py ties the roofline counters to those files' hashes).
#include <hip/hip_runtime.h>

#include "pbs_kernels.h"

namespace fhs {

// n pool blocks -> n consecutive rows (the inverse of scatter_blocks_kernel): one launch + ONE device-to-host copy bring
// a whole FheString back (fhs_download_string) instead of one synchronous 16 KB copy per block.
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint64_t *const *__restrict__ src, uint64_t *__restrict__ out) {
    const uint64_t *s = src[blockIdx.x];
    uint64_t *o = out + (size_t)blockIdx.x * BIG_CT;
    for (int e = threadIdx.x; e < BIG_CT; e += 256) o[e] = s[e];
}
hipError_t launch_gather_rows(const uint64_t *const *d_src, uint64_t *d_out, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(256), 0, s, d_src, d_out);
    return hipGetLastError();
}

// Pool compaction (fhs_pool_trim): workgroup g copies pool row src[g] to pool row dst[g].  A pool
// row is POOL_ROW_WORDS = 2050 words = 1025 pieces of 16 bytes on a 16-byte boundary, so every lane moves whole pieces
// (global_load_dwordx4 / global_store_dwordx4: 1 KiB contiguous per wavefront instruction): four per lane, all four
// loads in flight before the first store, and piece 1024 -- the body word, index 2048, with the padding word behind
// it -- by lane 0.  Sources and destinations are disjoint sets of rows (the caller's invariant): no ordering inside a
// launch matters.
static_assert(POOL_ROW_WORDS * 8 == (4 * 256 + 1) * 16, "a pool row is 4 pieces per lane and the tail piece");
__global__ __launch_bounds__(256) void pool_move_blocks_kernel(const uint64_t *const *__restrict__ src,
                                                               uint64_t *const *__restrict__ dst) {
    // (pointers read from a table are generic to the compiler: as global pointers they take global_* instead of flat_*)
    typedef uint32_t piece_t __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) piece_t *gsrc_t;
    typedef __attribute__((address_space(1))) piece_t *gdst_t;
    const gsrc_t s = (gsrc_t)src[blockIdx.x];
    const gdst_t d = (gdst_t)dst[blockIdx.x];
    const int t = threadIdx.x;
    const piece_t p0 = s[t], p1 = s[t + 256], p2 = s[t + 512], p3 = s[t + 768];
    piece_t tail = {0, 0, 0, 0};
    if (t == 0) tail = s[1024];
    d[t] = p0;
    d[t + 256] = p1;
    d[t + 512] = p2;
    d[t + 768] = p3;
    if (t == 0) d[1024] = tail;
}
hipError_t launch_pool_move_blocks(const uint64_t *const *d_src, uint64_t *const *d_dst, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pool_move_blocks_kernel, dim3(n), dim3(256), 0, s, d_src, d_dst);
    return hipGetLastError();
}

// User tables (fhs_user_lut): workgroup g writes the body polynomial of descriptor g -- what
// make_lut_poly (luts.h) computes on the host -- to dst + g * 2048.  Only the 16-byte descriptors travel, as kernel
// arguments; value x of a table is byte x of its descriptor.  Word i of the polynomial lies in box ((i + 64) / 128) mod 16
// (16 boxes of 128, rotated left by half a box) and the 64 words that wrapped round are negated.  A lane writes four
// 16-byte pieces (global_store_dwordx4, 1 KiB contiguous per wavefront instruction); the two words of a piece share
// their box because the rotation is even.  No load, no LDS.
static_assert(POLY_N == 2048 && POLY_N == 4 * 256 * 2, "four 16-byte pieces per lane");
__global__ __launch_bounds__(256) void expand_user_luts_kernel(UserLutBatch batch, uint64_t *__restrict__ dst) {
    typedef uint64_t piece_t __attribute__((ext_vector_type(2)));
    const uint64_t lo = batch.desc[blockIdx.x][0], hi = batch.desc[blockIdx.x][1];
    piece_t *o = reinterpret_cast<piece_t *>(dst + (size_t)blockIdx.x * POLY_N);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int p = j * 256 + threadIdx.x;                  // piece p = words 2p, 2p + 1
        const int q = 2 * p + POLY_N / 32;                    // ... of the unrotated polynomial, before the wrap
        const int box = (q >> 7) & 15;
        uint64_t v = (((box < 8 ? lo : hi) >> (8 * (box & 7))) & 31) << 59;
        if (q >= POLY_N) v = (uint64_t)0 - v;
        o[p] = piece_t{v, v};
    }
}
hipError_t launch_expand_user_luts(const uint8_t (*desc)[16], int n, uint64_t *d_dst, hipStream_t s) {
    for (int at = 0; at < n; at += USER_LUT_BATCH) {
        const int cnt = n - at < USER_LUT_BATCH ? n - at : USER_LUT_BATCH;
        UserLutBatch b{};
        for (int g = 0; g < cnt; g++)
            for (int x = 0; x < 16; x++) b.desc[g][x >> 3] |= (uint64_t)(desc[at + g][x] & 31) << (8 * (x & 7));
        hipLaunchKernelGGL(expand_user_luts_kernel, dim3(cnt), dim3(256), 0, s, b, d_dst + (size_t)at * POLY_N);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace fhs
