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

std::vector<uint64_t> key_to_ntt(const uint64_t *key, size_t n_polys) {
    std::vector<uint64_t> key_ntt(n_polys * 2 * N);
    for (size_t pi = 0; pi < n_polys; pi++)
        for (int q = 0; q < 2; q++) torus_poly_to_ntt(key + pi * N, BSK_QUANT_BITS, ntt_prime(q), key_ntt.data() + (pi * 2 + q) * N);
    return key_ntt;
}

void keyswitch_sums(const uint64_t *key_ntt, int L, const int64_t *digits, uint64_t *ks_mask, uint64_t *ks_body) {
    std::vector<uint64_t> buf((size_t)(2 * L + 4) * N);
    uint64_t *dig = buf.data() /* [prime][L] */, *acc = dig + (size_t)2 * L * N /* [col][prime] */;
    for (unsigned n = 0; n < N; n++)
        for (int l = 0; l < L; l++)
            for (int q = 0; q < 2; q++) dig[((size_t)q * L + l) * N + n] = to_residue(digits[(size_t)n * L + l], ntt_prime(q).p);
    for (int q = 0; q < 2; q++) {
        const NttPrime &pt = ntt_prime(q);
        for (int l = 0; l < L; l++) ntt_forward(dig + ((size_t)q * L + l) * N, pt);
        for (int c = 0; c < 2; c++) {
            uint64_t *a = acc + ((size_t)c * 2 + q) * N;
            for (unsigned n = 0; n < N; n++) {
                uint64_t s = 0;
                for (int l = 0; l < L; l++)
                    s += pt.mul(dig[((size_t)q * L + l) * N + n], key_ntt[((((size_t)l * 2 + c) * 2 + q) * N) + n]);
                a[n] = s % pt.p;
            }
            ntt_inverse(a, pt);
        }
    }
    // CRT to the centred integer, back to the torus: << 6 (the key was divided by 2^6)
    const NttPrime &p1 = ntt_prime(1);
    static const uint64_t crt = p1.pow(NTT_P0 % NTT_P1, NTT_P1 - 2);   // p0^-1 mod p1
    for (int c = 0; c < 2; c++)
        for (unsigned n = 0; n < N; n++) {
            const uint64_t r0 = acc[((size_t)c * 2 + 0) * N + n], r1 = acc[((size_t)c * 2 + 1) * N + n];
            const uint64_t r0m = r0 % NTT_P1;
            const uint64_t k = p1.mul(r1 >= r0m ? r1 - r0m : r1 + NTT_P1 - r0m, crt);
            const int64_t kc = k > NTT_P1 / 2 ? (int64_t)k - (int64_t)NTT_P1 : (int64_t)k;
            (c ? ks_body : ks_mask)[n] = (r0 + NTT_P0 * (uint64_t)kc) << BSK_QUANT_BITS;
        }
}

}  // namespace fhs
