#include "ntt_tables.h"

#include "host_ntt.h"
#include "host_parallel.h"
#include "pbs_kernels.h"

namespace fhs {
namespace {
inline double centred(uint64_t v, uint64_t p) { return v > p / 2 ? -(double)(p - v) : (double)v; }
}  // namespace

void build_ntt_tables(HostNttTables &t) {
    t.fwd_uni.assign(2 * 32, 0.0);
    t.fwd_lane.assign(2 * 32 * 64, 0.0);
    t.inv_uni.assign(2 * 64, 0.0);
    t.inv_lane.assign(2 * 32 * 64, 0.0);
    for (int q = 0; q < 2; q++) {
        const NttPrime &pt = ntt_prime(q);
        for (int k = 0; k < 32; k++) t.fwd_uni[q * 32 + k] = centred(pt.psi_br[k], pt.p);
        for (int k = 0; k < 64; k++) t.inv_uni[q * 64 + k] = centred(pt.ipsi_br[k], pt.p);
        for (int lane = 0; lane < 64; lane++) {
            t.fwd_lane[(q * 32 + 0) * 64 + lane] = centred(pt.psi_br[32 + lane / 2], pt.p);
            for (int e = 1; e < 32; e++) {
                int G = 1;
                while (2 * G <= e) G *= 2;
                const int g = e - G;
                const int idx = 64 * G + G * lane + g;
                t.fwd_lane[(q * 32 + e) * 64 + lane] = centred(pt.psi_br[idx], pt.p);
                t.inv_lane[(q * 32 + e) * 64 + lane] = centred(pt.ipsi_br[idx], pt.p);
            }
        }
    }
    t.crt_c = centred(ntt_prime(1).pow(NTT_P0 % NTT_P1, NTT_P1 - 2), NTT_P1);
    t.mono.assign(2 * 4096, 0.0);
    for (int q = 0; q < 2; q++) {
        const NttPrime &pt = ntt_prime(q);
        uint64_t a = 1;
        for (int k = 0; k < 4096; k++) {
            t.mono[q * 4096 + k] = centred(a, pt.p);
            a = pt.mul(a, pt.psi);
        }
    }
}

// The slot at array index idx of the device's forward transform holds the evaluation at psi^(2 bitrev11(idx) + 1):
// checked once per process on the monomial X (Context::load_multibit_key refuses to run otherwise).
bool ntt_slot_roots_are_bitreversed() {
    for (int q = 0; q < 2; q++) {
        const NttPrime &pt = ntt_prime(q);
        std::vector<uint64_t> a(POLY_N, 0);
        a[1] = 1;
        ntt_forward(a.data(), pt);
        for (unsigned idx = 0; idx < (unsigned)POLY_N; idx++)
            if (a[idx] != pt.pow(pt.psi, 2 * bitrev11(idx) + 1)) return false;
    }
    return true;
}

void convert_bsk_to_ntt(const uint64_t *bsk_std, double *out, int n_ggsw, int quant_bits) {
    convert_polys_to_ntt(bsk_std, out, (size_t)n_ggsw * 4, quant_bits);
}

void convert_polys_to_ntt(const uint64_t *polys, double *out, size_t n_polys, int quant_bits) {
    parallel_for(n_polys, host_threads(32), 1, [&](size_t pi) {
        std::vector<uint64_t> a(POLY_N);
        for (int q = 0; q < 2; q++) {
            const NttPrime &pt = ntt_prime(q);
            torus_poly_to_ntt(polys + pi * POLY_N, quant_bits, pt, a.data());
            double *dst = out + (pi * 2 + q) * POLY_N;
            for (int idx = 0; idx < POLY_N; idx++) {   // the device's contiguous layout: lane-major pairs of slots
                const int lane = idx >> 5, c = idx & 31;
                dst[((c >> 1) * 64 + lane) * 2 + (c & 1)] = centred(a[idx], pt.p);
            }
        }
    });
}

}  // namespace fhs
