// The GLWE keyswitch on the exact two-prime NTT of the blind rotation (ntt_transform.h), between a kernel's loads and its
// stores: the packing tree's automorphism keyswitch (pack_kernels.hip, three digits) and the three re-key kernels
// (rekey_kernels.hip, two digits) differ in where the digits come from and what is stored, not in this arithmetic.
// Host reference with the same words: keyswitch_sums of host_ntt.cpp.
#pragma once
#include "ntt_transform.h"

namespace fhs {

#pragma clang fp contract(off)

// One workgroup of 4 wavefronts; wavefront (j, q) = (wave >> 1, wave & 1) owns output polynomial j (0 mask, 1 body)
// modulo prime q.  What a wave needs of that, computed once: its LDS region and its sibling's (the other prime of the
// same polynomial), its prime and its twiddles.  A kernel builds it where it likes -- the packing tree before its gather,
// which is the order its registers were tuned in.
struct KeyswitchWave {
    int lane, j, q;
    double *my;
    const double *sibling;
    double p, pinv, p1, p1inv, twA, twB;
    const double *fwd_lane, *inv_lane;
    __device__ __forceinline__ KeyswitchWave(const NttTables &tw, char *smem, int lane_, int wave)
        : lane(lane_), j(wave >> 1), q(wave & 1) {
        my = reinterpret_cast<double *>(smem) + wave * LDS_WAVE_SLOTS;
        sibling = reinterpret_cast<double *>(smem) + (wave ^ 1) * LDS_WAVE_SLOTS;
        p = q ? (double)NTT_P1 : (double)NTT_P0;
        pinv = 1.0 / p;
        p1 = (double)NTT_P1;
        p1inv = 1.0 / p1;
        fwd_lane = tw.fwd_lane + q * 32 * 64;
        inv_lane = tw.inv_lane + q * 32 * 64;
        twA = lane < 32 ? C_FWD_UNI[q][lane] : C_INV_UNI[q][lane];
        twB = C_INV_UNI[q][lane & 31];
    }
};

// digit(r, l) is signed 16-bit digit l (0 = most significant) of the input mask's coefficient lane + 64 r, as a double;
// key_ntt is [sets][LEVELS][mask, body][prime][16][64 lanes][2], pre-scaled by N^-1, of which set key_set is used (the
// packing key has one set per tree level).  Every wave transforms all LEVELS digit polynomials under its prime (the two
// waves of a prime duplicate that work) and returns ks[o] = (sum_l d_l (*) K[l][j]) of coefficient lane + 64 (2 o + q),
// the half of output polynomial j that it owns, as a 64-bit torus word.  Holds the workgroup's one barrier: every load
// the caller made before the call is behind it on return, so the caller may store over its source.  `w` and the re-key
// kernels' digit lambda go by value: by reference those kernels take three more VGPRs (docs/HISTORY.md).
template <int LEVELS, class Digit>
__device__ __forceinline__ void glwe_keyswitch_sums(const KeyswitchWave w, Digit digit, const double *key_ntt, int key_set,
                                                    uint64_t (&ks)[16]) {
    const int lane = w.lane, j = w.j, q = w.q;
    const double p = w.p, pinv = w.pinv;

    // sum over the digits of NTT(d_l) * NTT(K[l][j]) modulo p
    typedef double __attribute__((ext_vector_type(2))) double2_t;
    double acc[32];
#pragma unroll
    for (int c = 0; c < 32; c++) acc[c] = 0.0;
#pragma unroll
    for (int l = 0; l < LEVELS; l++) {
        double x[32];
#pragma unroll
        for (int r = 0; r < 32; r++) x[r] = digit(r, l);
        __builtin_amdgcn_wave_barrier();
        ntt_forward(x, w.my, lane, w.twA, w.fwd_lane, p, pinv);
        // key layout [16][64 lanes][2]: one 16-byte load per lane covers coefficients (c, c + 1) of the contiguous layout
        const double2_t *key = reinterpret_cast<const double2_t *>(
            key_ntt + (((((size_t)key_set * LEVELS + l) * 2 + j) * 2 + q) * POLY_N)) + lane;
#pragma unroll
        for (int c = 0; c < 32; c += 2) {
            const double2_t kv = key[(c >> 1) * 64];
            const double m0 = mulmod(x[c], kv.x, p, pinv), m1 = mulmod(x[c + 1], kv.y, p, pinv);
            acc[c] += m0;
            acc[c + 1] += m1;
        }
    }
#pragma unroll
    for (int c = 0; c < 32; c++) acc[c] = reduce_once(acc[c], p, pinv);   // LEVELS products: back inside the inverse's input range
    __builtin_amdgcn_wave_barrier();
    ntt_inverse(acc, w.my, lane, w.twA, w.twB, w.inv_lane, p, pinv);
    __builtin_amdgcn_wave_barrier();

    // exchange residues with the other prime's wave, CRT for the owned half (coefficients lane + 64 (2 o + q))
    uint64_t *my_u = reinterpret_cast<uint64_t *>(w.my);
#pragma unroll
    for (int o = 0; o < 16; o++) ks[o] = 0;
    if (q == 0) phase_publish_residues<0>(acc, w.my, lane);
    else phase_publish_residues<1>(acc, w.my, lane);
    __syncthreads();                                  // ... and every wave's loads of the mask are behind it: stores may begin
    if (q == 0) phase_crt<0>(acc, ks, w.sibling, my_u, lane, C_CRT, w.p1, w.p1inv);
    else phase_crt<1>(acc, ks, w.sibling, my_u, lane, C_CRT, w.p1, w.p1inv);
}

// dynamic LDS of a kernel that calls glwe_keyswitch_sums: one transform region per wavefront
inline size_t keyswitch_lds_bytes() { return (size_t)4 * LDS_WAVE_SLOTS * sizeof(double); }

}  // namespace fhs
