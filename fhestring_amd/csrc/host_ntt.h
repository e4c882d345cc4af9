// The exact host NTT over the device's two primes (pbs_kernels.h: NTT_P0 / NTT_P1, psi a primitive 4096-th root):
// negacyclic transforms of Z_p[X]/(X^2048+1) in the flow of the device kernels.  One copy for the key conversion of
// ntt_tables.cpp and for the packing reference of pack_host.cpp; any exact method gives the same words.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fhs {

struct NttPrime {
    uint64_t p, psi, barrett;               // barrett = floor(2^94 / p)
    std::vector<uint64_t> psi_br, ipsi_br;  // psi^bitrev(k), psi^-bitrev(k)
    uint64_t ninv;                          // 1/2048 mod p
    // a, b < p < 2^47: a b mod p with one 96-bit quotient estimate (at most three corrections)
    uint64_t mul(uint64_t a, uint64_t b) const {
        const unsigned __int128 x = (unsigned __int128)a * b;
        const uint64_t q = (uint64_t)(((unsigned __int128)(uint64_t)(x >> 46) * barrett) >> 48);
        uint64_t r = (uint64_t)(x - (unsigned __int128)q * p);
        while (r >= p) r -= p;
        return r;
    }
    uint64_t pow(uint64_t b, uint64_t e) const;
};
const NttPrime &ntt_prime(int q);   // q = 0, 1

inline unsigned bitrev11(unsigned x) {
    unsigned r = 0;
    for (int i = 0; i < 11; i++) r |= ((x >> i) & 1u) << (10 - i);
    return r;
}
// negacyclic forward (Cooley-Tukey, natural order in; slot idx holds the evaluation at psi^(2 bitrev11(idx) + 1)) and
// inverse (Gentleman-Sande, without 1/N), in place on 2048 residues
void ntt_forward(uint64_t *a, const NttPrime &t);
void ntt_inverse(uint64_t *a, const NttPrime &t);

inline uint64_t to_residue(int64_t v, uint64_t p) {
    const int64_t m = v % (int64_t)p;
    return (uint64_t)(m < 0 ? m + (int64_t)p : m);
}
// the closest multiple of 2^bits (ties upwards, modulo 2^64): the grid of the bootstrapping and packing keys
inline uint64_t round_to_grid(uint64_t x, int bits) { return (x + (1ull << (bits - 1))) & ~((1ull << bits) - 1); }

// Key material in the transform domain: out[idx] = NTT(signed(round_to_grid(poly, quant_bits)) / 2^quant_bits mod p)[idx] / N
// for the 2048 torus words of `poly`, slots in the order of ntt_forward.
void torus_poly_to_ntt(const uint64_t *poly, int quant_bits, const NttPrime &t, uint64_t *out);

// ---- the GLWE keyswitch of the packing tree and of the re-key family (pack_host.cpp, rekey_host.cpp; device:
// glwe_keyswitch.h), on a key of 16-bit digit levels on the bootstrapping key's grid ----
constexpr int KEYSWITCH_BASE_LOG = 16;
// signed digits of the closest multiple of 2^(64 - 16 L) to x, most significant first (l = 0), each in [-2^15, 2^15);
// a carry out of the top digit is a multiple of 2^64
inline void decompose(uint64_t x, int L, int64_t *d) {
    const int sh = 64 - L * KEYSWITCH_BASE_LOG;
    uint64_t v = (x + (1ull << (sh - 1))) >> sh;
    uint64_t carry = 0;
    for (int l = L - 1; l >= 0; l--) {
        int64_t dg = (int64_t)((v & ((1ull << KEYSWITCH_BASE_LOG) - 1)) + carry);
        v >>= KEYSWITCH_BASE_LOG;
        if (dg >= (int64_t)1 << (KEYSWITCH_BASE_LOG - 1)) { dg -= (int64_t)1 << KEYSWITCH_BASE_LOG; carry = 1; }
        else carry = 0;
        d[l] = dg;
    }
}
// a keyswitch key of n_polys torus polynomials as residues: [n_polys][prime][2048], rounded to the 58-bit grid, 1/N
// folded in (torus_poly_to_ntt)
std::vector<uint64_t> key_to_ntt(const uint64_t *key, size_t n_polys);
// the 64-bit keyswitch sums of one GLWE mask before any rounding: ks_mask / ks_body[2048] = sum_l d_l (*) K[l].col with
// digits[n * L + l] = digit l of coefficient n (decompose) and key_ntt = [L][mask, body][prime][2048]
void keyswitch_sums(const uint64_t *key_ntt, int L, const int64_t *digits, uint64_t *ks_mask, uint64_t *ks_body);

}  // namespace fhs
