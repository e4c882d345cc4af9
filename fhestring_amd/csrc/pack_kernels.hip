// Packed result download on gfx950: ring packing of up to 2048 LWE blocks into one GLWE (Chen, Dai, Kim, Song,
// Alg. PackLWEs) with the exact two-prime NTT of the blind rotation (ntt_transform.h), then a 16-bit storage switch.
// DESIGN.md section 11; host reference with the same words: pack_host.cpp.
//
// One launch per tree level lv = 1..11, one workgroup (4 wavefronts) per live node: with the children E (even blocks) and
// O (odd blocks), t = N >> lv and g = 2^lv + 1,
//     T = X^t O,  P = E + T,  M = E - T,  out = P + AutoKS_g(M),
//     AutoKS_g(A, B) = (-sum_l d_l (*) K_g[l].mask,  B(X^g) - sum_l d_l (*) K_g[l].body),  d = digits of A(X^g).
// Wavefront (j, q) owns output polynomial j (0 mask, 1 body) modulo prime q, as in blind_rotate_kernel.  The monomial
// shift and the automorphism are index arithmetic on the loads (a gather, no scatter): coefficient n of A(X^g) is
// +-A[n g^-1 mod 2N].  Every wave decomposes A(X^g) itself and transforms all three digit polynomials under its prime (the
// two waves of a prime duplicate that work: the simplest mapping, and the whole packing is a few blind rotations' worth).
// Level 1 reads the pool blocks through a table, divides by N with rounding and builds the leaf GLWE
// (A_0 = a_0, A_{N-i} = -a_i, B = b) on the fly.
#include "glwe_keyswitch.h"
#include "pack_kernels.h"
#include "storage_words.h"

namespace fhs {

#pragma clang fp contract(off)

namespace {

struct PackChild {
    const uint64_t *p;   // GLWE in the workspace, or (leaf) the pool block / nullptr for a trivial block
    uint64_t body;       // leaf, p == nullptr: body of the trivial block
    bool live;
};

__device__ __forceinline__ uint64_t pack_prescale(uint64_t x) { return (x + (1ull << 10)) >> 11; }

// coefficient m of polynomial col (0 mask, 1 body) of a child
template <bool LEAF>
__device__ __forceinline__ uint64_t child_coef(const PackChild &c, int col, uint32_t m) {
    if (!c.live) return 0;
    if (!LEAF) return c.p[col * POLY_N + m];
    if (col == 0) {
        if (!c.p) return 0;
        return m == 0 ? pack_prescale(c.p[0]) : (uint64_t)0 - pack_prescale(c.p[POLY_N - m]);
    }
    return m == 0 ? pack_prescale(c.p ? c.p[BIG_N] : c.body) : 0;
}
// coefficient i of P = E + X^t O and of M = E - X^t O
template <bool LEAF>
__device__ __forceinline__ void node_pm(const PackChild &E, const PackChild &O, int col, uint32_t i, uint32_t t,
                                        uint64_t &P, uint64_t &M) {
    const uint64_t ev = child_coef<LEAF>(E, col, i);
    uint64_t tv = child_coef<LEAF>(O, col, (i - t) & (POLY_N - 1));
    if (i < t) tv = (uint64_t)0 - tv;
    P = ev + tv;
    M = ev - tv;
}
// coefficient n of M(X^g): +-M[i], i = n g^-1 mod 2N
template <bool LEAF>
__device__ __forceinline__ uint64_t node_auto(const PackChild &E, const PackChild &O, int col, uint32_t n, uint32_t t,
                                              uint32_t ginv) {
    const uint32_t i2 = (n * ginv) & (2 * POLY_N - 1);
    uint64_t P, M;
    node_pm<LEAF>(E, O, col, i2 & (POLY_N - 1), t, P, M);
    return i2 >= (uint32_t)POLY_N ? (uint64_t)0 - M : M;
}
// signed digit l (0 = most significant) of the closest multiple of 2^16 to x, base 2^16, digits in [-2^15, 2^15): adding
// 0x8000 at every lower digit position carries into digit k exactly when the balanced lower digits do
__device__ __forceinline__ double pack_digit(uint64_t x, int l) {
    const uint64_t v = (x + (1ull << (63 - PACK_LEVELS * PACK_BASE_LOG))) >> (64 - PACK_LEVELS * PACK_BASE_LOG);
    const int k = PACK_LEVELS - 1 - l;
    const uint64_t h = k == 0 ? 0 : (k == 1 ? 0x8000ull : 0x80008000ull);
    return (double)(int16_t)(uint16_t)((v + h) >> (PACK_BASE_LOG * k));
}
static_assert(PACK_LEVELS == 3 && PACK_BASE_LOG == 16, "pack_digit is written for three 16-bit digits");

}  // namespace

template <bool LEAF>
__global__ __launch_bounds__(256) void pack_level_kernel(PackLevelParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t n_lv = (uint32_t)POLY_N >> P.lv;
    const uint32_t grp = blockIdx.y, k = blockIdx.x;
    const uint32_t count = min((uint32_t)PACK_GROUP, P.total - grp * PACK_GROUP);
    if (k >= min(count, n_lv)) return;            // uniform for the workgroup: node not live
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = wave >> 1;   // output polynomial (0 mask, 1 body)
    const int q = wave & 1;    // prime
    const KeyswitchWave kw(P.tw, smem, lane, wave);

    // children: nodes k (even blocks) and k + n_lv (odd blocks) of the level below; at level 1 they are blocks
    PackChild E, O;
    E.live = true;
    O.live = k + n_lv < count;
    E.body = O.body = 0;
    if (LEAF) {
        const PackLeaf *lf = P.leaves + (size_t)grp * PACK_GROUP;
        E.p = lf[k].blk; E.body = lf[k].body;
        O.p = nullptr;
        if (O.live) { O.p = lf[k + n_lv].blk; O.body = lf[k + n_lv].body; }
    } else {
        const uint64_t *src = P.src + (size_t)grp * 2 * n_lv * 2 * POLY_N;
        E.p = src + (size_t)k * 2 * POLY_N;
        O.p = src + (size_t)(k + n_lv) * 2 * POLY_N;
    }
    const uint32_t t = n_lv;                       // N / 2^lv
    const uint32_t g = (1u << P.lv) + 1;
    uint32_t ginv = g;                             // g^-1 mod 2N: Newton steps double the correct low bits (3 -> 6 -> 12 -> 24)
    ginv *= 2 - g * ginv;
    ginv *= 2 - g * ginv;
    ginv *= 2 - g * ginv;

    // A(X^g) of M's mask, strided layout: a1[r] = coefficient lane + 64 r
    uint64_t a1[32];
#pragma unroll
    for (int r = 0; r < 32; r++) a1[r] = node_auto<LEAF>(E, O, 0, lane + 64 * r, t, ginv);

    // ks = sum_l d_l (*) K_g[l][j] of this wave's half of polynomial j (glwe_keyswitch.h; it holds the workgroup's barrier)
    uint64_t ks[16];
    glwe_keyswitch_sums<PACK_LEVELS>(kw, [&a1](int r, int l) { return pack_digit(a1[r], l); }, P.key_ntt, P.lv - 1, ks);

    // out = P + AutoKS(M): mask P_A - sum, body P_B + B(X^g) - sum
    uint64_t *out = P.dst + ((size_t)grp * n_lv + k) * 2 * POLY_N + (size_t)j * POLY_N;
#pragma unroll
    for (int o = 0; o < 16; o++) {
        const uint32_t n = lane + 64 * (2 * o + q);
        uint64_t Pn, Mn;
        node_pm<LEAF>(E, O, j, n, t, Pn, Mn);
        uint64_t v = Pn - ks[o];
        if (j == 1) v += node_auto<LEAF>(E, O, 1, n, t, ginv);
        out[n] = v;
    }
}

hipError_t prepare_device_for_packing() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(pack_level_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)keyswitch_lds_bytes());
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(pack_level_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)keyswitch_lds_bytes());
}

hipError_t launch_pack_level(const PackLevelParams &p, hipStream_t s) {
    if (!fills_groups(p.total, p.groups, PACK_GROUP) || p.lv < 1 || p.lv > PACK_TREE_LEVELS) return hipErrorInvalidValue;
    const uint32_t n_lv = (uint32_t)POLY_N >> p.lv;
    const dim3 grid(p.groups > 1 ? n_lv : (p.total < n_lv ? p.total : n_lv), p.groups);
    if (p.lv == 1) hipLaunchKernelGGL(pack_level_kernel<true>, grid, dim3(256), keyswitch_lds_bytes(), s, p);
    else hipLaunchKernelGGL(pack_level_kernel<false>, grid, dim3(256), keyswitch_lds_bytes(), s, p);
    return hipGetLastError();
}

// ---- storage switch: every word of the packed GLWE -> round16 (storage_words.h) ----
__global__ __launch_bounds__(256) void pack_switch16_kernel(const uint64_t *__restrict__ glwe, uint16_t *__restrict__ mask16,
                                                            uint16_t *__restrict__ body16, uint32_t total) {
    const uint32_t grp = blockIdx.x;
    const uint32_t count = min((uint32_t)PACK_GROUP, total - grp * PACK_GROUP);
    const uint64_t *a = glwe + (size_t)grp * 2 * POLY_N, *b = a + POLY_N;
    for (uint32_t i = threadIdx.x; i < (uint32_t)POLY_N; i += 256) {
        mask16[(size_t)grp * POLY_N + i] = round16(a[i]);
        if (i < count) body16[(size_t)grp * PACK_GROUP + i] = round16(b[i]);
    }
}
hipError_t launch_pack_switch16(const uint64_t *d_glwe, uint16_t *d_mask16, uint16_t *d_body16, int groups, uint32_t total,
                                hipStream_t s) {
    if (!fills_groups(total, groups, PACK_GROUP)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_switch16_kernel, dim3(groups), dim3(256), 0, s, d_glwe, d_mask16, d_body16, total);
    return hipGetLastError();
}

}  // namespace fhs
