// Launchers of seeded_kernels.hip: masks of compressed (seeded) ciphertexts and server keys regenerated on the device
// from their public ChaCha20 seed (the convention of include/fhestring_hip.h, "compressed ciphertexts and keys").
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace fhs {

struct SeedKey { uint32_t w[8]; };   // 256-bit ChaCha20 key: the public seed

// n pool blocks of one seeded string: block j is the string's global block first_block + j (= 4 x character + digit,
// its ChaCha20 stream id).  d_desc = [n bodies][n destination pointers]: mask (2048 draws) and body go straight into the
// destination block.
hipError_t launch_expand_seeded_blocks(const SeedKey &seed, uint64_t first_block, const uint64_t *d_desc, int n,
                                       hipStream_t s);
// standard-domain BSK [742][2][2][2048]: mask polynomials from the seed (& the 58-bit grid), bodies [742][2][2048]
hipError_t launch_expand_seeded_bsk(const SeedKey &seed, const uint64_t *d_bodies, uint64_t *d_bsk, hipStream_t s);
// KSK [2048][5][743]: 742 draws per row from the seed, bodies [2048][5]
hipError_t launch_expand_seeded_ksk(const SeedKey &seed, const uint64_t *d_bodies, uint64_t *d_ksk, hipStream_t s);
// n 64-bit draws of the keystream (key, counter, nonce), the generator's own counter carry included (diagnostic)
hipError_t launch_chacha20_stream(const SeedKey &key, uint32_t counter, const uint32_t nonce[3], uint64_t *d_out,
                                  size_t n, hipStream_t s);

}  // namespace fhs
