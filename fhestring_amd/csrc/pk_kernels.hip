// Public-key uploads (include/fhestring_hip.h, "public-key encryption"): a group of up to 2048
// blocks arrives as one GLWE ciphertext stored at 32 bits, and block j of the group is its sample extraction at
// coefficient j,  a_i = A[j - i] (i <= j),  -A[2048 + j - i] (i > j),  b = B[j],  every word widened by << 32.
// 16 392 B written per block against 8 KB of mask read per GROUP: store-bound, like expand_seeded_blocks_kernel, and
// not part of any bootstrap (kept out of the profiled kernel sources).
#include <hip/hip_runtime.h>

#include "../../include/fhestring_hip.h"
#include "pbs_kernels.h"
#include "pk_kernels.h"

namespace fhs {

namespace {

// One workgroup per PK_BLOCKS_PER_WG consecutive coefficients of one group (2048 is a multiple of it, so a workgroup
// never straddles two groups).  The group's mask is staged once in LDS as the signed, unrolled sequence
//   g[k] = -A[k + 1] (k < 2047),   g[k] = A[k - 2047] (2047 <= k < 4095)      so that      a_i = g[j - i + 2047]:
// the rotation, the reversal and the negation become one descending index, with no wrap-around.  g is kept split by the
// parity of k (even | odd halves): lane t's 16-byte store holds words 2c, 2c + 1 (c = 256 q + t), i.e. g[p] and g[p - 1]
// with p = j + 2047 - 2c, which are element (p >> 1) of one half and ((p - 1) >> 1) of the other -- consecutive lanes
// read consecutive descending dwords of each half (ds_read_b32, 32 banks: conflict-free).  Every store instruction of a
// wavefront covers 1 KiB contiguous; pool rows are 16-byte aligned (2050-word stride), as in the seeded kernel.
__global__ __launch_bounds__(256) void expand_public_blocks_kernel(const uint32_t *__restrict__ masks,
                                                                   const uint32_t *__restrict__ bodies,
                                                                   uint64_t *const *__restrict__ dst, uint32_t first_coef,
                                                                   int n) {
    __shared__ uint32_t g[2 * BIG_N];
    const int t = threadIdx.x;
    // pass-local block k has group-relative coefficient first_coef + k (first_coef < 2048; a pass may run on into the
    // next groups, whose masks follow in `masks`)
    const uint32_t c0 = (first_coef / PK_BLOCKS_PER_WG + blockIdx.x) * PK_BLOCKS_PER_WG;   // this workgroup's first coefficient
    const uint32_t *a = masks + (size_t)(c0 / BIG_N) * BIG_N;
    for (int k = t; k < 2 * BIG_N; k += 256) {
        uint32_t v = 0;
        if (k < BIG_N - 1) v = 0u - a[k + 1];
        else if (k < 2 * BIG_N - 1) v = a[k - (BIG_N - 1)];
        g[(k & 1) * BIG_N + (k >> 1)] = v;
    }
    __syncthreads();
    for (int b = 0; b < PK_BLOCKS_PER_WG; b++) {
        const int k = (int)(c0 + b) - (int)first_coef;          // pass-local block (uniform over the workgroup)
        if (k < 0 || k >= n) continue;
        const int j = (int)((c0 + b) % BIG_N);
        uint64_t *row = dst[k];
        uint4 *o = reinterpret_cast<uint4 *>(row);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = q * 256 + t, p = j + (BIG_N - 1) - 2 * c;      // 1 <= p <= 4094
            const uint32_t w0 = g[(p & 1) * BIG_N + (p >> 1)], w1 = g[((p - 1) & 1) * BIG_N + ((p - 1) >> 1)];
            o[c] = make_uint4(0u, w0, 0u, w1);
        }
        if (t == 0) row[BIG_N] = (uint64_t)bodies[k] << 32;
    }
}

}  // namespace

hipError_t launch_expand_public_blocks(const uint32_t *d_masks, const uint32_t *d_bodies, uint64_t *const *d_dst,
                                       uint32_t first_coef, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (first_coef >= (uint32_t)BIG_N) return hipErrorInvalidValue;
    const uint32_t wgs = (first_coef + (uint32_t)n - 1) / PK_BLOCKS_PER_WG - first_coef / PK_BLOCKS_PER_WG + 1;
    hipLaunchKernelGGL(expand_public_blocks_kernel, dim3(wgs), dim3(256), 0, s, d_masks, d_bodies, d_dst, first_coef, n);
    return hipGetLastError();
}

}  // namespace fhs
