#include "host_ntt.h"

#include "pbs_kernels.h"

namespace fhs {
namespace {
constexpr unsigned N = POLY_N;

NttPrime make_prime(uint64_t p, uint64_t psi) {
    NttPrime t;
    t.p = p;
    t.psi = psi;
    t.barrett = (uint64_t)((((unsigned __int128)1) << 94) / p);
    t.psi_br.resize(N);
    t.ipsi_br.resize(N);
    const uint64_t ipsi = t.pow(psi, p - 2);
    uint64_t a = 1, b = 1;
    for (unsigned i = 0; i < N; i++) {
        t.psi_br[bitrev11(i)] = a;
        t.ipsi_br[bitrev11(i)] = b;
        a = t.mul(a, psi);
        b = t.mul(b, ipsi);
    }
    t.ninv = t.pow(N, p - 2);
    return t;
}
}  // namespace

uint64_t NttPrime::pow(uint64_t b, uint64_t e) const {
    uint64_t r = 1;
    for (; e; e >>= 1, b = mul(b, b))
        if (e & 1) r = mul(r, b);
    return r;
}

const NttPrime &ntt_prime(int q) {
    static const NttPrime t0 = make_prime(NTT_P0, NTT_PSI0), t1 = make_prime(NTT_P1, NTT_PSI1);
    return q ? t1 : t0;
}

void ntt_forward(uint64_t *a, const NttPrime &t) {
    const uint64_t p = t.p;
    unsigned len = N;
    for (unsigned m = 1; m < N; m <<= 1) {
        len >>= 1;
        for (unsigned i = 0; i < m; i++) {
            const uint64_t w = t.psi_br[m + i];
            uint64_t *x = a + 2 * i * len, *y = x + len;
            for (unsigned k = 0; k < len; k++) {
                const uint64_t u = x[k], v = t.mul(y[k], w);
                x[k] = u + v >= p ? u + v - p : u + v;
                y[k] = u >= v ? u - v : u + p - v;
            }
        }
    }
}

void ntt_inverse(uint64_t *a, const NttPrime &t) {
    const uint64_t p = t.p;
    unsigned len = 1;
    for (unsigned m = N / 2; m >= 1; m >>= 1) {
        for (unsigned i = 0; i < m; i++) {
            const uint64_t w = t.ipsi_br[m + i];
            uint64_t *x = a + 2 * i * len, *y = x + len;
            for (unsigned k = 0; k < len; k++) {
                const uint64_t u = x[k], v = y[k];
                x[k] = u + v >= p ? u + v - p : u + v;
                y[k] = t.mul(u >= v ? u - v : u + p - v, w);
            }
        }
        len <<= 1;
    }
}

void torus_poly_to_ntt(const uint64_t *poly, int quant_bits, const NttPrime &t, uint64_t *out) {
    for (unsigned n = 0; n < N; n++) out[n] = to_residue((int64_t)round_to_grid(poly[n], quant_bits) >> quant_bits, t.p);
    ntt_forward(out, t);
    for (unsigned n = 0; n < N; n++) out[n] = t.mul(out[n], t.ninv);
}

}  // namespace fhs
