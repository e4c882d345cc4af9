// The ChaCha20 block function (RFC 8439) on the device, shared by seeded_kernels.hip (compressed ciphertexts and server
// keys) and select_kernels.hip (seeded select queries): the stream layout of the client's generator (client.cpp, Rng):
// key = seed, st[12] = block counter from 0, st[13] = domain, st[14] / st[15] = stream id low / high, draw k = words
// (2k, 2k + 1) of the keystream, low word first.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "seeded_kernels.h"

namespace fhs {

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

#define FHS_DQR(a, b, c, d)                          \
    x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 16);    \
    x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 12);    \
    x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 8);     \
    x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 7);

// One ChaCha20 block, bit-equal to Rng::refill's scalar path.  out[j] = draw j of the block (8 per block).
__device__ __forceinline__ void chacha20_block(const SeedKey &k, uint32_t ctr, uint32_t n13, uint32_t n14, uint32_t n15,
                                               uint64_t out[8]) {
    const uint32_t st[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, k.w[0], k.w[1], k.w[2], k.w[3],
                             k.w[4],      k.w[5],      k.w[6],      k.w[7],      ctr,    n13,    n14,    n15};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = st[i];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        FHS_DQR(0, 4, 8, 12) FHS_DQR(1, 5, 9, 13) FHS_DQR(2, 6, 10, 14) FHS_DQR(3, 7, 11, 15)
        FHS_DQR(0, 5, 10, 15) FHS_DQR(1, 6, 11, 12) FHS_DQR(2, 7, 8, 13) FHS_DQR(3, 4, 9, 14)
    }
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = (uint64_t)(x[2 * j] + st[2 * j]) | ((uint64_t)(x[2 * j + 1] + st[2 * j + 1]) << 32);
}
#undef FHS_DQR

}  // namespace fhs
