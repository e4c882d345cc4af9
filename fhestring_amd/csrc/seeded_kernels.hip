// Compressed (seeded) ciphertexts and server keys: the uniform masks are regenerated on the device from the public
// 256-bit seed, ChaCha20 (RFC 8439 block function) with the stream layout of the client's generator (client.cpp, Rng):
// key = seed, st[12] = block counter from 0, st[13] = domain, st[14] / st[15] = stream id low / high, draw k = words
// (2k, 2k + 1) of the keystream, low word first (the block function: chacha_device.h).  Not part of any bootstrap
// (kept out of the profiled kernel sources).
#include <hip/hip_runtime.h>

#include "../../include/fhestring_hip.h"
#include "chacha_device.h"
#include "pbs_kernels.h"
#include "seeded_kernels.h"

namespace fhs {

namespace {

// One workgroup per ciphertext, one thread per 64-byte keystream block: thread t makes mask words 8t .. 8t + 7.  The
// workgroup's 16 KiB are staged through LDS so that every store instruction writes 1 KiB contiguous per wavefront (16 B
// per lane); each thread storing its own 64 bytes directly (four strided 16-byte stores) measured 2 % slower
// (profiles/r07_compressed_store_ab.txt).
__global__ __launch_bounds__(256) void expand_seeded_blocks_kernel(SeedKey seed, uint64_t first_block,
                                                                   const uint64_t *__restrict__ desc, int n) {
    __shared__ uint64_t stage[BIG_N];
    const int j = blockIdx.x, t = threadIdx.x;
    uint64_t *dst = reinterpret_cast<uint64_t *const *>(desc + n)[j];
    const uint64_t stream = first_block + (uint64_t)j;
    uint64_t w[8];
    chacha20_block(seed, (uint32_t)t, FHS_DOM_SEEDED_STR, (uint32_t)stream, (uint32_t)(stream >> 32), w);
    ulonglong2 *l = reinterpret_cast<ulonglong2 *>(stage + 8 * t);
#pragma unroll
    for (int q = 0; q < 4; q++) l[q] = make_ulonglong2(w[2 * q], w[2 * q + 1]);
    __syncthreads();
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(stage);
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(dst);   // pool rows are 16-byte aligned (POOL_STRIDE 2050)
#pragma unroll
    for (int q = 0; q < 4; q++) o[q * 256 + t] = src[q * 256 + t];
    if (t == 0) dst[BIG_N] = desc[j];
}

// BSK: one workgroup per GGSW row (key bit i, row r: stream 2i + r), thread t = keystream block t of that row
__global__ __launch_bounds__(256) void expand_seeded_bsk_kernel(SeedKey seed, const uint64_t *__restrict__ bodies,
                                                                uint64_t *__restrict__ bsk) {
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const uint64_t qmask = ~((1ull << BSK_QUANT_BITS) - 1);
    uint64_t w[8];
    chacha20_block(seed, t, FHS_DOM_SEEDED_BSK, p, 0, w);
    uint64_t *mask = bsk + (size_t)p * 2 * POLY_N, *body = mask + POLY_N;
    const uint64_t *b = bodies + (size_t)p * POLY_N;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        mask[8 * t + q] = w[q] & qmask;
        body[8 * t + q] = b[8 * t + q];
    }
}

// KSK: row (i, l) = stream 5i + l, 742 draws = 93 keystream blocks (the last two draws of the 93rd are not used)
constexpr int KSK_ROWS = BIG_N * KS_LEVEL;
constexpr int KSK_BLOCKS_PER_ROW = (LWE_N + 7) / 8;
__global__ __launch_bounds__(256) void expand_seeded_ksk_kernel(SeedKey seed, const uint64_t *__restrict__ bodies,
                                                                uint64_t *__restrict__ ksk) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= (uint32_t)KSK_ROWS * KSK_BLOCKS_PER_ROW) return;
    const uint32_t row = g / KSK_BLOCKS_PER_ROW, c = g % KSK_BLOCKS_PER_ROW;
    uint64_t w[8];
    chacha20_block(seed, c, FHS_DOM_SEEDED_KSK, row, 0, w);
    uint64_t *ct = ksk + (size_t)row * SMALL_CT;
#pragma unroll
    for (int q = 0; q < 8; q++)
        if (8 * c + q < (uint32_t)LWE_N) ct[8 * c + q] = w[q];
    if (c == 0) ct[LWE_N] = bodies[row];
}

// diagnostic keystream: block g of (key, counter, nonce); the counter's carry goes into st[13] above the domain byte
// (+0x100), as in Rng::refill
__global__ __launch_bounds__(256) void chacha20_stream_kernel(SeedKey key, uint32_t counter, uint32_t n0, uint32_t n1,
                                                              uint32_t n2, uint64_t *__restrict__ out, uint64_t n) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (8 * g >= n) return;
    const uint64_t c = (uint64_t)counter + g;
    uint64_t w[8];
    chacha20_block(key, (uint32_t)c, n0 + 0x100u * (uint32_t)(c >> 32), n1, n2, w);
    for (int q = 0; q < 8; q++)
        if (8 * g + q < n) out[8 * g + q] = w[q];
}

}  // namespace

hipError_t launch_expand_seeded_blocks(const SeedKey &seed, uint64_t first_block, const uint64_t *d_desc, int n,
                                       hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(expand_seeded_blocks_kernel, dim3(n), dim3(256), 0, s, seed, first_block, d_desc, n);
    return hipGetLastError();
}

hipError_t launch_expand_seeded_bsk(const SeedKey &seed, const uint64_t *d_bodies, uint64_t *d_bsk, hipStream_t s) {
    hipLaunchKernelGGL(expand_seeded_bsk_kernel, dim3(LWE_N * 2), dim3(256), 0, s, seed, d_bodies, d_bsk);
    return hipGetLastError();
}

hipError_t launch_expand_seeded_ksk(const SeedKey &seed, const uint64_t *d_bodies, uint64_t *d_ksk, hipStream_t s) {
    const int threads = KSK_ROWS * KSK_BLOCKS_PER_ROW;
    hipLaunchKernelGGL(expand_seeded_ksk_kernel, dim3((threads + 255) / 256), dim3(256), 0, s, seed, d_bodies, d_ksk);
    return hipGetLastError();
}

hipError_t launch_chacha20_stream(const SeedKey &key, uint32_t counter, const uint32_t nonce[3], uint64_t *d_out,
                                  size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 7) / 8;
    hipLaunchKernelGGL(chacha20_stream_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, key, counter,
                       nonce[0], nonce[1], nonce[2], d_out, (uint64_t)n);
    return hipGetLastError();
}

}  // namespace fhs
