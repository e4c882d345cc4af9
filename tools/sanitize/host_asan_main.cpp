// ASan/UBSan driver of the product's HOST-ONLY code (no device is touched): client keygen / encrypt / decrypt /
// key files (client.cpp), public-key encryption and its expansion (pk_host.cpp), the exact host NTT (host_ntt.cpp), the twiddle and key transforms (ntt_tables.cpp, fft_tables.cpp), and the whole DAG layer --
// engine.cpp graph logic, radix.cpp, strings*.cpp, capi_*.cpp -- through a planner context (fhs_ctx_create_planner),
// which records and levelises every string op of the C ABI without executing anything.
// Built by `make -C fhestring_amd/csrc asan`; run by tests/test_sanitizers.py.  CPU only.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fhestring_hip.h"
#include "../../fhestring_amd/csrc/fft_tables.h"
#include "../../fhestring_amd/csrc/host_ntt.h"
#include "../../fhestring_amd/csrc/keyfile.h"
#include "../../fhestring_amd/csrc/ntt_tables.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("CHECK failed: %s (line %d)\n", #x, __LINE__); fails++; } } while (0)

static std::vector<fhs_char_t> dummy(fhs_ctx *c, size_t n) {
    std::vector<uint64_t> z((size_t)FHS_CHAR_WORDS, 0);
    std::vector<fhs_char_t> v;
    for (size_t i = 0; i < n; i++) v.push_back(fhs_upload(c, z.data()));
    return v;
}

int main() {
    uint64_t res0[5], res1[5];
    CHECK(fhs_debug_live_resources(res0) == FHS_OK && fhs_debug_live_resources(nullptr) == FHS_ERR_ARG);
    // ---- client -----------------------------------------------------------------------------------------------
    fhs_client *ck = nullptr;
    CHECK(fhs_client_create_insecure_seeded(42, &ck) == FHS_OK);
    std::vector<uint64_t> ct((size_t)12 * FHS_CHAR_WORDS);
    CHECK(fhs_client_encrypt_str(ck, "sanitizers", 10, 2, ct.data()) == FHS_OK);
    char buf[16];
    size_t n = 0;
    CHECK(fhs_client_decrypt_str(ck, ct.data(), 12, buf, &n) == FHS_OK && n == 10 && !std::memcmp(buf, "sanitizers", 10));
    CHECK(fhs_client_encrypt_str(ck, "bad\0x", 5, 0, ct.data()) == FHS_ERR_ARG);
    const std::string path = "/tmp/fhs_asan_key.bin";
    CHECK(fhs_client_save(ck, path.c_str(), 0) == FHS_OK);
    fhs_client *ck2 = nullptr;
    CHECK(fhs_client_load(path.c_str(), &ck2) == FHS_OK);
    uint8_t v = 0;
    CHECK(fhs_client_decrypt_char(ck2, ct.data(), &v) == FHS_OK);
    fhs_client *os = nullptr;
    CHECK(fhs_client_create(&os) == FHS_OK);           // OS-entropy path
    fhs_client_destroy(os);
    {   // public-key encryption and its host expansion (pk_host.cpp): a string that crosses a group boundary
        uint32_t seed[8];
        std::vector<uint64_t> body(FHS_PK_BODY_WORDS);
        CHECK(fhs_client_public_key(ck, seed, body.data()) == FHS_OK);
        const std::string pub = "/tmp/fhs_asan_public.bin";
        CHECK(fhs_client_save_public_key(ck, pub.c_str()) == FHS_OK);
        void *pk = nullptr, *pk2 = nullptr, *none = nullptr;
        fhs_client *no_client = nullptr;
        CHECK(fhs_public_key_load(pub.c_str(), &pk) == FHS_OK && fhs_public_key_create(seed, body.data(), &pk2) == FHS_OK);
        CHECK(fhs_client_load(pub.c_str(), &no_client) != FHS_OK && fhs_public_key_load(path.c_str(), &none) != FHS_OK);   // kinds 6 / 1
        std::remove(pub.c_str());
        CHECK(fhs_public_key_set_insecure_seed(pk, 5) == FHS_OK);
        const std::string text(515, 's');
        size_t mw = 0, bw = 0;
        fhs_public_str_words(text.size() + 2, &mw, &bw);
        CHECK(mw == 2 * 2048 && bw == 4 * 517);
        std::vector<uint32_t> m32(mw), b32(bw);
        CHECK(fhs_public_encrypt_str(pk, text.data(), text.size(), 2, m32.data(), b32.data()) == FHS_OK);
        CHECK(fhs_public_encrypt_str(pk, "bad\0x", 5, 0, m32.data(), b32.data()) == FHS_ERR_ARG);
        std::vector<uint64_t> win((size_t)10 * FHS_CHAR_WORDS);
        CHECK(fhs_expand_public_str(m32.data(), b32.data(), 517, 507, 10, win.data()) == FHS_OK);   // blocks 2028 .. 2067
        CHECK(fhs_expand_public_str(m32.data(), b32.data(), 517, 510, 10, win.data()) == FHS_ERR_ARG);
        char pbuf[16];
        size_t pn = 0;
        CHECK(fhs_client_decrypt_str(ck, win.data(), 10, pbuf, &pn) == FHS_OK && pn == 8 && !std::memcmp(pbuf, "ssssssss", 8));
        {   // a row fetched by encrypted index on the host (select_host.cpp): 640 characters in rows of 128 -- two groups, the
            // second partial, one tree level and two rotates -- and the refusals
            std::string table;
            for (int r = 0; r < 5; r++) table += std::string(128, (char)('a' + r));
            std::vector<uint32_t> tm(2 * 2048), tb(4 * 640), rm(2048), rb(4 * 128);
            CHECK(fhs_public_encrypt_str(pk, table.data(), table.size(), 0, tm.data(), tb.data()) == FHS_OK);
            const int bits = fhs_store_select_bits(640, 128);
            CHECK(bits == 3 && fhs_store_select_bits(640, 96) == 0 && fhs_store_select_bits(128, 128) == 0);
            std::vector<uint64_t> q(FHS_SELECT_QUERY_WORDS(bits));
            CHECK(fhs_client_select_query(ck, 4, bits, q.data()) == FHS_OK && fhs_client_select_query(ck, 4, 0, q.data()) == FHS_ERR_ARG);
            CHECK(fhs_store_select_host(q.data(), bits, tm.data(), tb.data(), 4 * 640, 128, rm.data(), rb.data()) == FHS_OK);
            std::vector<uint64_t> row((size_t)128 * FHS_CHAR_WORDS);
            std::vector<char> rbuf(129);
            CHECK(fhs_expand_public_str(rm.data(), rb.data(), 128, 0, 128, row.data()) == FHS_OK);
            CHECK(fhs_client_decrypt_str(ck, row.data(), 128, rbuf.data(), &pn) == FHS_OK && pn == 128 &&
                  std::string(rbuf.data(), 128) == std::string(128, 'e'));
            CHECK(fhs_store_select_host(q.data(), 2, tm.data(), tb.data(), 4 * 640, 128, rm.data(), rb.data()) == FHS_ERR_ARG);
            CHECK(fhs_store_select_host(q.data(), bits, tm.data(), tb.data(), 4 * 640, 1024, rm.data(), rb.data()) == FHS_ERR_ARG);
            CHECK(fhs_store_select_host(nullptr, bits, tm.data(), tb.data(), 4 * 640, 128, rm.data(), rb.data()) == FHS_ERR_ARG);
        }
        {   // that compact string re-keyed to a second client, in place (rekey_host.cpp); the re-key key and its kind 7 file
            fhs_client *to = nullptr;
            CHECK(fhs_client_create_insecure_seeded(43, &to) == FHS_OK);
            std::vector<uint64_t> rk(FHS_REKEY_KEY_WORDS), rk2;
            CHECK(fhs_client_rekey_key(ck, to, rk.data()) == FHS_OK && fhs_client_rekey_key(ck, nullptr, rk.data()) == FHS_ERR_ARG);
            {   // ... and widened to 64-bit GLWEs, as a packed download for that client (fhs_rekey_packed_host)
                std::vector<uint64_t> m64(mw), b64(mw, 0);
                for (size_t i = 0; i < mw; i++) m64[i] = (uint64_t)m32[i] << 32;
                for (size_t i = 0; i < bw; i++) b64[i] = (uint64_t)b32[i] << 32;
                std::vector<uint16_t> m16(mw), b16(bw);
                std::vector<char> all(518);
                CHECK(fhs_rekey_packed_host(rk.data(), m64.data(), b64.data(), bw, m16.data(), b16.data()) == FHS_OK);
                CHECK(fhs_client_decrypt_packed_str(to, m16.data(), b16.data(), 517, all.data(), &pn) == FHS_OK && pn == 515 &&
                      !std::memcmp(all.data(), text.data(), 515));
                CHECK(fhs_rekey_packed_host(rk.data(), nullptr, nullptr, 4, nullptr, nullptr) == FHS_ERR_ARG);
            }
            {   // ... and a window across its two groups as the packed download of a parked entry, own key and for that
                // client (fhs_store_packed_host): output arrays of exactly the window's size
                size_t wmw = 0, wbw = 0;
                uint32_t fc = 0;
                fhs_store_packed_words(511, 6, &wmw, &wbw, &fc);
                CHECK(wmw == 2 * 2048 && wbw == 24 && fc == 2044);
                std::vector<uint16_t> m16(wmw), b16(wbw);
                char w[8];
                CHECK(fhs_store_packed_host(nullptr, m32.data(), b32.data(), bw, 511, 6, m16.data(), b16.data()) == FHS_OK);
                CHECK(fhs_client_decrypt_packed_str_at(ck, m16.data(), b16.data(), fc, 6, w, &pn) == FHS_OK && pn == 4 &&
                      !std::memcmp(w, text.data() + 511, 4));
                CHECK(fhs_store_packed_host(rk.data(), m32.data(), b32.data(), bw, 511, 6, m16.data(), b16.data()) == FHS_OK);
                CHECK(fhs_client_decrypt_packed_str_at(to, m16.data(), b16.data(), fc, 6, w, &pn) == FHS_OK && pn == 4 &&
                      !std::memcmp(w, text.data() + 511, 4));
                CHECK(fhs_store_packed_host(nullptr, m32.data(), b32.data(), bw, 512, 6, m16.data(), b16.data()) == FHS_ERR_ARG);
                CHECK(fhs_client_decrypt_packed_str_at(ck, m16.data(), b16.data(), 2, 6, w, &pn) == FHS_ERR_ARG);
            }
            CHECK(fhs_rekey_host(rk.data(), m32.data(), b32.data(), bw, m32.data(), b32.data()) == FHS_OK);
            CHECK(fhs_expand_public_str(m32.data(), b32.data(), 517, 507, 10, win.data()) == FHS_OK);
            CHECK(fhs_client_decrypt_str(to, win.data(), 10, pbuf, &pn) == FHS_OK && pn == 8 && !std::memcmp(pbuf, "ssssssss", 8));
            CHECK(fhs_client_save_rekey_key(ck, to, pub.c_str()) == FHS_OK && fhs_read_rekey_key_file(pub.c_str(), rk2) == FHS_OK &&
                  rk2.size() == FHS_REKEY_KEY_WORDS);
            CHECK(fhs_read_packing_key_file(pub.c_str(), rk2) == FHS_ERR_STATE);                     // kind 7
            std::remove(pub.c_str());
            fhs_client_destroy(to);
        }
        fhs_public_key_destroy(pk);
        fhs_public_key_destroy(pk2);
    }
    {   // the key-file readers (keyfile.h) return what the writers were given; a file that cannot be opened is an error
        const std::string kf = "/tmp/fhs_asan_kind.bin";
        std::vector<uint64_t> a, b;
        uint32_t seed[8], cseed[8];
        CHECK(fhs_read_server_key_file(path.c_str(), a, b) == FHS_OK && a.size() == FHS_BSK_WORDS && b.size() == FHS_KSK_WORDS);
        CHECK(!std::memcmp(a.data(), fhs_client_bsk(ck), a.size() * 8) && !std::memcmp(b.data(), fhs_client_ksk(ck), b.size() * 8));
        CHECK(fhs_client_save(ck, kf.c_str(), 1) == FHS_OK && fhs_read_server_key_file(kf.c_str(), a, b) == FHS_OK);
        CHECK(!std::memcmp(a.data(), fhs_client_bsk(ck), a.size() * 8) && !std::memcmp(b.data(), fhs_client_ksk(ck), b.size() * 8));
        CHECK(fhs_client_save_multibit_key(ck, kf.c_str()) == FHS_OK && fhs_read_multibit_key_file(kf.c_str(), a) == FHS_OK);
        CHECK(a.size() == FHS_BSK_MB2_WORDS && !std::memcmp(a.data(), fhs_client_bsk_mb2(ck), a.size() * 8));
        std::vector<uint64_t> bb(FHS_CBSK_BODY_WORDS), kb(FHS_CKSK_BODY_WORDS);
        CHECK(fhs_client_compressed_server_key(ck, cseed, bb.data(), kb.data()) == FHS_OK);
        CHECK(fhs_client_save_compressed_server_key(ck, kf.c_str()) == FHS_OK &&
              fhs_read_compressed_server_key_file(kf.c_str(), seed, a, b) == FHS_OK);
        CHECK(!std::memcmp(seed, cseed, 32) && a == bb && b == kb);
        CHECK(fhs_client_save_packing_key(ck, kf.c_str()) == FHS_OK && fhs_read_packing_key_file(kf.c_str(), a) == FHS_OK);
        CHECK(a.size() == FHS_PACK_KEY_WORDS && !std::memcmp(a.data(), fhs_client_packing_key(ck), a.size() * 8));
        CHECK(fhs_read_multibit_key_file(kf.c_str(), b) == FHS_ERR_STATE);                         // kind 5
        CHECK(fhs_client_public_key(ck, cseed, bb.data()) == FHS_OK && fhs_client_save_public_key(ck, kf.c_str()) == FHS_OK);
        CHECK(fhs_read_public_key_file(kf.c_str(), seed, a) == FHS_OK && !std::memcmp(seed, cseed, 32) && a.size() == 2048 &&
              !std::memcmp(a.data(), bb.data(), 2048 * 8));
        std::remove(kf.c_str());
        CHECK(fhs_read_public_key_file(kf.c_str(), seed, a) == FHS_ERR_STATE);
        CHECK(fhs_client_save(ck, "/nonexistent-directory/key.bin", 0) == FHS_ERR_STATE);
    }
    std::remove(path.c_str());

    // ---- host transforms of the key ---------------------------------------------------------------------------
    {
        fhs::HostNttTables ht;
        fhs::build_ntt_tables(ht);
        fhs::HostFftTables ft;
        fhs::build_fft_tables(ft);
        CHECK(ht.fwd_uni.size() == 64 && ft.w_re.size() == 1024 && ft.mono.size() == 2 * 4096 && ft.r16.size() == 32);
        const uint64_t *mb = fhs_client_bsk_mb2(ck);              // pair key of FHS_ARITH_F64_FFT_MB2 (generated here)
        CHECK(mb != nullptr && (mb[0] & 63) == 0 && fhs_client_bsk_mb2(ck) == mb);
        std::vector<double> out((size_t)4 * 2 * 2 * 2048);       // one GGSW
        std::vector<uint64_t> one(fhs_client_bsk(ck), fhs_client_bsk(ck) + 4 * 2048);
        // convert_bsk_to_ntt walks all 742 GGSWs: give it the real key (reads only)
        std::vector<double> all((size_t)742 * 4 * 2 * 2048);
        fhs::convert_bsk_to_ntt(fhs_client_bsk(ck), all.data());
    }

    // ---- host NTT (host_ntt.h): chosen inputs, both primes ---------------------------------------------------------
    for (int q = 0; q < 2; q++) {
        using namespace fhs;
        constexpr unsigned N = 2048;
        const NttPrime &pt = ntt_prime(q);
        const uint64_t p = pt.p;
        uint64_t lcg = 0x9E3779B97F4A7C15ull + (uint64_t)q;
        auto rnd = [&] { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (lcg >> 11) % p; };
        std::vector<uint64_t> r(N), edge(N, 0);
        for (auto &x : r) x = rnd();
        edge[0] = edge[1] = edge[N - 1] = p - 1;
        // (a) forward, inverse, times 1/N: the identity
        for (const std::vector<uint64_t> *in : {&r, &edge}) {
            std::vector<uint64_t> a(*in);
            ntt_forward(a.data(), pt);
            ntt_inverse(a.data(), pt);
            for (auto &x : a) x = pt.mul(x, pt.ninv);
            CHECK(a == *in);
        }
        // (b) the transform product with a 16-term polynomial against the schoolbook negacyclic product mod p
        const unsigned at[16] = {0, 1, 2, 3, 17, 100, 511, 512, 1023, 1024, 1025, 1500, 1999, 2045, 2046, 2047};
        std::vector<uint64_t> s16(N, 0), want(N, 0), fa(r), fb;
        for (unsigned j : at) s16[j] = rnd();
        for (unsigned j : at)
            for (unsigned i = 0; i < N; i++) {
                const uint64_t t = pt.mul(r[i], s16[j]);
                uint64_t &w = want[(i + j) % N];
                w = i + j < N ? (w + t) % p : (w + p - t) % p;
            }
        fb = s16;
        ntt_forward(fa.data(), pt);
        ntt_forward(fb.data(), pt);
        for (unsigned i = 0; i < N; i++) fa[i] = pt.mul(pt.mul(fa[i], fb[i]), pt.ninv);
        ntt_inverse(fa.data(), pt);
        CHECK(fa == want);
    }
    {   // (c) convert_polys_to_ntt on monomials: the device layout and the rounding to the key grid
        using namespace fhs;
        constexpr unsigned N = 2048;
        struct Case { uint64_t coeff; unsigned k; int quant_bits; bool zero; };
        const Case cases[] = {{1ull << 6, 0, 6, false}, {1ull << 6, 1, 6, false}, {1ull << 6, 2047, 6, false},
                              {1ull << 7, 1, 7, false}, {1ull << 5, 1, 6, false}, {(1ull << 5) - 1, 1, 6, true}};
        for (const Case &cs : cases) {
            std::vector<uint64_t> poly(N, 0);
            std::vector<double> out(2 * N, -1.0);
            poly[cs.k] = cs.coeff;
            convert_polys_to_ntt(poly.data(), out.data(), 1, cs.quant_bits);
            int bad = 0;
            for (int q = 0; q < 2; q++) {
                const NttPrime &pt = ntt_prime(q);
                for (unsigned idx = 0; idx < N; idx++) {
                    const unsigned lane = idx >> 5, c = idx & 31;
                    const uint64_t v = pt.mul(pt.pow(pt.psi, (uint64_t)(2 * bitrev11(idx) + 1) * cs.k % 4096), pt.ninv);
                    const double want = cs.zero ? 0.0 : v > pt.p / 2 ? -(double)(pt.p - v) : (double)v;
                    bad += out[(size_t)q * N + ((c >> 1) * 64 + lane) * 2 + (c & 1)] != want;
                }
            }
            CHECK(bad == 0);
        }
    }

    // ---- DAG layer through the planner ------------------------------------------------------------------------
    fhs_ctx *c = nullptr;
    CHECK(fhs_ctx_create_planner(&c) == FHS_OK);
    // strings whose characters are mostly PLAINTEXT (trivial) with a few ciphertexts in between: sums fold, trees see
    // constants, noise-driven groupings see zero-variance terms -- the shapes on which fixed-size term buffers overflowed
    auto mixed = [&](size_t n, size_t every) {
        std::vector<uint64_t> z((size_t)FHS_CHAR_WORDS, 0);
        std::vector<fhs_char_t> v;
        for (size_t i = 0; i < n; i++) v.push_back(i % every == every / 2 ? fhs_upload(c, z.data()) : fhs_trivial(c, (uint8_t)("ab c"[i % 4])));
        return v;
    };
    {   // the parser of regex_clear alone: valid patterns, malformed ones cut short at every place, the limits
        size_t positions = 0, low = 0, off = 0;
        CHECK(fhs_regex_info("(error|warn).*timeout", 21, FHS_REGEX_IGNORE_CASE, &positions, &low, &off) == FHS_OK && positions == 17 && low == 11);
        CHECK(fhs_regex_info("a{64}", 5, 0, &positions, &low, nullptr) == FHS_OK && positions == 64 && low == 64);
        CHECK(fhs_regex_info("a{64}", 5, FHS_REGEX_SEARCH, &positions, &low, &off) == FHS_ERR_LIMIT);
        CHECK(fhs_regex_info(nullptr, 0, FHS_REGEX_SEARCH, &positions, nullptr, nullptr) == FHS_OK && positions == 2);
        CHECK(fhs_regex_info("(a|b", 4, 0, nullptr, nullptr, &off) == FHS_ERR_ARG && off == 0);
        CHECK(fhs_regex_info("ab[c-", 5, 0, nullptr, nullptr, &off) == FHS_ERR_ARG && off == 2);
        CHECK(fhs_regex_info("ab\\", 3, 0, nullptr, nullptr, &off) == FHS_ERR_ARG && off == 2);
        CHECK(fhs_regex_info("a{1,", 4, 0, nullptr, nullptr, &off) == FHS_ERR_ARG && off == 1);
        CHECK(fhs_regex_info("a{99999999999999999999}", 23, 0, nullptr, nullptr, nullptr) == FHS_ERR_LIMIT);
        // long patterns whose trees would be deep: refused by the written-size limit before anything walks them
        for (const char *unit : {"|", "a", "()", "a|", "(?:)|", "a?"})
            for (size_t bytes : {(size_t)4096, (size_t)200000}) {
                std::string big;
                while (big.size() < bytes) big += unit;
                CHECK(fhs_regex_info(big.data(), big.size(), FHS_REGEX_SEARCH, &positions, &low, &off) == FHS_ERR_LIMIT && off == 0);
            }
        {
            const std::string nested = std::string(65, '(') + "a" + std::string(65, ')');
            CHECK(fhs_regex_info(nested.data(), nested.size(), 0, nullptr, nullptr, nullptr) == FHS_ERR_LIMIT);
            const std::string bars(1000, '|');                           // within the limit: 1001 empty branches
            CHECK(fhs_regex_info(bars.data(), bars.size(), 0, &positions, &low, nullptr) == FHS_OK && positions == 0 && low == 0);
        }
        const char *full = "x(?:a|[^b-d\\x41\\d]){2,3}\\.\\x4a+|(y*)?";
        for (size_t cut = 0; cut <= std::strlen(full); cut++)            // every prefix: accepted or refused, never read past
            for (uint32_t fl = 0; fl < 4; fl++) {
                std::vector<char> exact(full, full + cut);               // (a buffer of exactly `cut` bytes)
                const int rc = fhs_regex_info(exact.data(), cut, fl, &positions, &low, &off);
                CHECK(rc == FHS_OK || (rc == FHS_ERR_ARG && off <= cut));
            }
    }
    for (int variant = 0; variant < 5; variant++)
    for (int mode = 0; mode < 2; mode++) {
        if (variant >= 3 && mode == 0) continue;                 // long strings: the re-associated DAGs only (as written is O(n^2) nodes)
        CHECK(fhs_set_mode(c, mode) == FHS_OK);
        auto s = variant == 0 ? dummy(c, 14) : variant == 1 ? mixed(14, 5) : variant == 2 ? mixed(40, 9) : variant == 3 ? mixed(200, 50) : mixed(254, 300);
        auto p = variant == 0 ? dummy(c, 3) : mixed(3, variant == 1 ? 2 : 7), to = variant == 0 ? dummy(c, 5) : mixed(5, 3);
        auto o = variant == 0 ? dummy(c, 14) : mixed(s.size() - (variant & 1), 11);
        fhs_char_t r = 0, f = 0;
        CHECK(fhs_str_contains(c, s.data(), s.size(), p.data(), p.size(), &r) == FHS_OK);
        CHECK(fhs_str_contains_clear(c, s.data(), s.size(), "abc", 3, &r) == FHS_OK);
        // LIKE: every token kind, segments of every position, escapes, both case modes; the malformed patterns
        for (const char *pat : {"", "%", "a%", "%c", "%ab%", "ab c%b_", "a%b%c%_", "_%_", "%%a%%", "ab cab cab cab cab c%", "a!%b!_!!%"})
            for (uint32_t fl = 0; fl < 2; fl++)
                CHECK(fhs_str_like_clear(c, s.data(), s.size(), pat, std::strlen(pat), '!', fl, &r) == FHS_OK && r);
        CHECK(fhs_str_like_clear(c, s.data(), s.size(), "a\0b", 3, -1, 0, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_like_clear(c, s.data(), s.size(), "ab!", 3, '!', 0, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_like_clear(c, s.data(), s.size(), "ab", 2, '%', 0, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_like_clear(c, s.data(), s.size(), "ab", 2, -1, 2, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_like_clear(c, s.data(), s.size(), "ab", 2, -1, 0, nullptr) == FHS_ERR_ARG);
        // regular expressions: every construct, every flag combination; patterns the parser decides alone; the refused ones
        for (const char *pat : {"", "ab c", "a.*c", "(ab| c)+a?", "[a-c ]{2,3}.*", "[^b]+", "\\w+\\s\\S*", "(a|b|c| |ab|bc|c a|abc)*", ".*",
                                "a{0}(b{2,}|[\\x61-\\x63]?)*", "(ab c){3}ab.*", "\\0?a.*"})
            for (uint32_t fl = 0; fl < 4; fl++)
                CHECK(fhs_str_regex_clear(c, s.data(), s.size(), pat, std::strlen(pat), fl, &r) == FHS_OK && r);
        CHECK(fhs_str_regex_clear(c, s.data(), s.size(), "a\0b", 3, 0, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_regex_clear(c, s.data(), s.size(), "(ab", 3, 0, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_regex_clear(c, s.data(), s.size(), "a{65}", 5, 0, &r) == FHS_ERR_LIMIT);
        CHECK(fhs_str_regex_clear(c, s.data(), s.size(), "ab", 2, 4, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_regex_clear(c, s.data(), s.size(), "ab", 2, 0, nullptr) == FHS_ERR_ARG);
        // ... and where they match: the automaton run backwards, the position in both widths and the flags of all starts
        for (const char *pat : {"", "ab c", "a.*c", "(ab| c)+a?", "[a-c ]{2,3}.*", "[^b]+", "\\w+\\s\\S*", "(a|b|c| |ab|bc|c a|abc)+",
                                "a{0}(b{2,}|[\\x61-\\x63]?)*", "(ab c){3}ab.*", "\\0?a.*"})
            for (uint32_t fl = 0; fl < 2; fl++) {
                std::vector<fhs_char_t> starts(s.size() + 1, 0);
                fhs_char_t lo = 0, hi = 0;
                CHECK(fhs_str_regex_find_clear(c, s.data(), s.size(), pat, std::strlen(pat), fl, &r) == FHS_OK && r);
                CHECK(fhs_str_regex_find_clear_wide(c, s.data(), s.size(), pat, std::strlen(pat), fl, &lo, &hi) == FHS_OK && lo && hi);
                CHECK(fhs_str_regex_starts_clear(c, s.data(), s.size(), pat, std::strlen(pat), fl, starts.data()) == FHS_OK && starts[s.size() - 1]);
                CHECK(starts[s.size()] == 0);
            }
        CHECK(fhs_str_regex_find_clear(c, s.data(), s.size(), "ab", 2, FHS_REGEX_SEARCH, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_regex_starts_clear(c, s.data(), s.size(), "(ab", 3, 0, &r) == FHS_ERR_ARG);
        CHECK(fhs_str_regex_find_clear_wide(c, s.data(), s.size(), "a{65}", 5, 0, &r, &f) == FHS_ERR_LIMIT);
        CHECK(fhs_str_starts_with(c, s.data(), s.size(), p.data(), p.size(), &r) == FHS_OK);
        CHECK(fhs_str_ends_with(c, s.data(), s.size(), p.data(), p.size(), &r) == FHS_OK);
        CHECK(fhs_str_find(c, s.data(), s.size(), p.data(), p.size(), &r) == FHS_OK);
        CHECK(fhs_str_rfind(c, s.data(), s.size(), p.data(), p.size(), &r) == FHS_OK);
        CHECK(fhs_str_is_empty(c, s.data(), s.size(), &r) == FHS_OK);
        CHECK(fhs_str_len(c, s.data(), s.size(), &r) == FHS_OK);
        {   // the 16-bit forms: (lo, hi) handles, the same strings and a flag vector
            fhs_char_t lo = 0, hi = 0;
            CHECK(fhs_str_find_wide(c, s.data(), s.size(), p.data(), p.size(), &lo, &hi) == FHS_OK && lo && hi);
            CHECK(fhs_str_find_clear_wide(c, s.data(), s.size(), "abc", 3, &lo, &hi) == FHS_OK);
            CHECK(fhs_str_rfind_wide(c, s.data(), s.size(), p.data(), p.size(), &lo, &hi) == FHS_OK);
            CHECK(fhs_str_rfind_wide(c, s.data(), s.size(), nullptr, 0, &lo, &hi) == FHS_OK);
            CHECK(fhs_str_len_wide(c, s.data(), s.size(), &lo, &hi) == FHS_OK);
            CHECK(fhs_flags_count_wide(c, s.data(), s.size(), &lo, &hi) == FHS_OK);
            if (mode == 1 && variant == 4) {                      // past the u8 limit: digits 4 to 7 get blocks
                auto big = mixed(1030, 40);
                CHECK(fhs_str_find_wide(c, big.data(), big.size(), p.data(), p.size(), &lo, &hi) == FHS_OK);
                CHECK(fhs_str_rfind_wide(c, big.data(), big.size(), p.data(), p.size(), &lo, &hi) == FHS_OK);
                CHECK(fhs_str_len_wide(c, big.data(), big.size(), &lo, &hi) == FHS_OK);
                CHECK(fhs_str_find(c, big.data(), big.size(), p.data(), p.size(), &r) == FHS_ERR_LIMIT);
            }
            CHECK(fhs_str_find_wide(c, s.data(), s.size(), p.data(), p.size(), nullptr, &hi) == FHS_ERR_ARG);
            // the positions as operands: find's noisy digits are refreshed on the way in, results of every length
            CHECK(fhs_str_find_wide(c, s.data(), s.size(), p.data(), p.size(), &lo, &hi) == FHS_OK);
            CHECK(fhs_str_find(c, s.data(), s.size(), p.data(), p.size(), &r) == FHS_OK);
            std::vector<fhs_char_t> head(s.size() + 5, 0), tail(s.size() + 5, 0);
            CHECK(fhs_str_char_at(c, s.data(), s.size(), r, &f) == FHS_OK && f);
            CHECK(fhs_str_char_at_wide(c, s.data(), s.size(), lo, hi, &f) == FHS_OK && f);
            CHECK(fhs_str_substr(c, s.data(), s.size(), r, s.size() + 5, head.data()) == FHS_OK && head.back());
            CHECK(fhs_str_substr_wide(c, s.data(), s.size(), lo, hi, 3, head.data()) == FHS_OK);
            CHECK(fhs_str_take(c, s.data(), s.size(), r, head.data()) == FHS_OK);
            CHECK(fhs_str_take_wide(c, s.data(), s.size(), lo, hi, head.data()) == FHS_OK);
            CHECK(fhs_str_split_at(c, s.data(), s.size(), r, head.data(), tail.data()) == FHS_OK);
            CHECK(fhs_str_split_at_wide(c, s.data(), s.size(), lo, hi, head.data(), tail.data()) == FHS_OK);
            CHECK(fhs_str_substr(c, s.data(), s.size(), r, 0, nullptr) == FHS_OK);
            CHECK(fhs_str_take(c, nullptr, 0, r, nullptr) == FHS_OK);
            CHECK(fhs_str_substr(c, s.data(), s.size(), r, 3, nullptr) == FHS_ERR_ARG);
            CHECK(fhs_str_split_at(c, s.data(), s.size(), 0, head.data(), tail.data()) == FHS_ERR_ARG);
        }
        CHECK(fhs_str_eq(c, s.data(), s.size(), o.data(), o.size(), &r) == FHS_OK);
        CHECK(fhs_str_ne(c, s.data(), s.size(), o.data(), o.size(), &r) == FHS_OK);
        CHECK(fhs_str_eq_ignore_case(c, s.data(), s.size(), o.data(), o.size(), &r) == FHS_OK);
        for (int cmp = 0; cmp < 4; cmp++) CHECK(fhs_str_compare(c, s.data(), s.size(), o.data(), o.size(), cmp, &r) == FHS_OK);
        std::vector<fhs_char_t> out(64 * 16 + 2 * s.size() + o.size(), 0);
        CHECK(fhs_str_to_upper(c, s.data(), s.size(), out.data()) == FHS_OK);
        CHECK(fhs_str_to_lower(c, s.data(), s.size(), out.data()) == FHS_OK);
        CHECK(fhs_str_trim(c, s.data(), s.size(), out.data()) == FHS_OK);
        CHECK(fhs_str_trim_start(c, s.data(), s.size(), out.data()) == FHS_OK);
        CHECK(fhs_str_trim_end(c, s.data(), s.size(), out.data()) == FHS_OK);
        CHECK(fhs_str_strip_prefix(c, s.data(), s.size(), p.data(), p.size(), out.data(), &f) == FHS_OK);
        CHECK(fhs_str_strip_suffix(c, s.data(), s.size(), p.data(), p.size(), out.data(), &f) == FHS_OK);
        size_t len = 0;
        std::vector<fhs_char_t> rep(fhs_str_replace_len(s.size(), p.size(), to.size()) + 8);
        CHECK(fhs_str_replace(c, s.data(), s.size(), p.data(), p.size(), to.data(), to.size(), rep.data(), rep.size(), &len) == FHS_OK);
        CHECK(fhs_str_replace(c, s.data(), s.size(), to.data(), to.size(), p.data(), p.size(), rep.data(), rep.size(), &len) == FHS_OK);
        CHECK(fhs_str_concatenate(c, s.data(), s.size(), o.data(), o.size(), out.data()) == FHS_OK);
        if (mode == 1 && variant < 3) {                           // (the split family allocates n x n handles)
            for (int kind = 0; kind < 9; kind++) {
                const size_t d = fhs_str_split_dim(kind, s.size());
                std::vector<fhs_char_t> sp(d * d);
                size_t dim = 0;
                fhs_char_t cnt = (kind == 3 || kind == 6) ? fhs_trivial(c, 2) : 0;
                CHECK(fhs_str_split(c, kind, s.data(), s.size(), p.data(), kind == 8 ? 0 : p.size(), cnt, sp.data(), sp.size(), &dim, &f) == FHS_OK);
            }
        }
        CHECK(fhs_flush(c) == FHS_OK);
        uint64_t blocks[FHS_CHAR_WORDS];
        CHECK(fhs_download(c, r, blocks) == FHS_ERR_STATE);      // a planner computes nothing
    }
    {   // string store on the planner: put, re-key in place and as a copy (bookkeeping only), get
        auto s = dummy(c, 3);
        uint64_t id = 0, id2 = 0, none = 7;
        uint32_t nk = 9;
        std::vector<fhs_char_t> back(3);
        CHECK(fhs_store_put(c, s.data(), s.size(), &id) == FHS_OK && fhs_store_rekey(c, id, nullptr) == FHS_OK);
        CHECK(fhs_store_rekey(c, id, &id2) == FHS_OK && id2 != 0 && id2 != id && fhs_store_rekey(c, id + 100, &none) == FHS_ERR_ARG && none == 0);
        CHECK(fhs_store_rekey_count(c, id, &nk) == FHS_OK && nk == 1);
        CHECK(fhs_store_get(c, id2, 0, 3, back.data()) == FHS_OK && fhs_store_drop(c, id) == FHS_OK && fhs_store_drop(c, id2) == FHS_OK);
        CHECK(fhs_load_rekey_key(c, nullptr) == FHS_OK && fhs_load_rekey_key_file(c, "/nonexistent-directory/key.bin") == FHS_ERR_STATE);
        uint16_t w16[4];
        CHECK(fhs_download_string_packed_for(c, s.data(), 0, nullptr, nullptr, nullptr, nullptr) == FHS_OK &&
              fhs_download_string_packed_for(c, s.data(), 1, w16, w16, nullptr, nullptr) == FHS_ERR_STATE);   // a planner
    }
    {   // level-skewed batching: jobs on ticks, dependent jobs, handles released while their levels are still scheduled
        CHECK(fhs_set_mode(c, 1) == FHS_OK);
        CHECK(fhs_resident_slots(c) == 512 && fhs_set_tick_balance(c, 64) == FHS_OK);   // levels get split across ticks
        CHECK(fhs_set_launch_chunk(c, 0, 100) == FHS_OK && fhs_set_launch_chunk(c, 7, 1) == FHS_ERR_ARG);
        std::vector<fhs_char_t> keep;
        for (int k = 0; k < 6; k++) {
            auto s = dummy(c, 30);
            fhs_char_t r = 0, f = 0;
            CHECK(fhs_str_contains_clear(c, s.data(), s.size(), "abc", 3, &r) == FHS_OK);
            CHECK(fhs_str_find_clear(c, s.data(), s.size(), "abc", 3, &f) == FHS_OK);
            CHECK(fhs_submit(c) == FHS_OK);
            for (fhs_char_t h : s) CHECK(fhs_release(c, h) == FHS_OK);      // inputs dropped before their ticks run
            if (k & 1) CHECK(fhs_release(c, f) == FHS_OK); else keep.push_back(f);
            if (!keep.empty() && k == 3) {                                   // a job consuming an unfinished job
                fhs_char_t e = fhs_eq(c, keep[0], r);
                CHECK(e != 0 && fhs_submit(c) == FHS_OK);
                keep.push_back(e);
            }
            keep.push_back(r);
            CHECK(fhs_pump(c, 1) == FHS_OK);
        }
        CHECK(fhs_flush(c) == FHS_OK);
        size_t nl = 0;
        CHECK(fhs_level_widths(c, nullptr, 0, &nl) == FHS_OK && nl > 20);
        for (fhs_char_t h : keep) CHECK(fhs_release(c, h) == FHS_OK);
        CHECK(fhs_set_tick_balance(c, 0) == FHS_OK);
    }
    {   // all-trivial inputs: every bootstrap folds at recording time (the CPU truth-table tests live on this path)
        CHECK(fhs_set_mode(c, 1) == FHS_OK);
        std::vector<fhs_char_t> s, p;
        for (int i = 0; i < 257; i++) s.push_back(fhs_trivial(c, i == 256 ? 0 : (uint8_t)('a' + i % 3)));
        for (char ch : std::string("wxyz")) p.push_back(fhs_trivial(c, (uint8_t)ch));
        fhs_char_t r = 0;
        int triv = 0;
        uint8_t val = 0;
        CHECK(fhs_str_find(c, s.data(), s.size(), p.data(), p.size(), &r) == FHS_OK);
        CHECK(fhs_trivial_value(c, r, &triv, &val) == FHS_OK && triv == 1 && val == 255);
        CHECK(fhs_str_rfind(c, s.data(), s.size(), p.data(), p.size(), &r) == FHS_OK);
        CHECK(fhs_trivial_value(c, r, &triv, &val) == FHS_OK && triv == 1 && val == 255);
        std::vector<fhs_char_t> out(s.size());
        CHECK(fhs_bubble_zeroes_right(c, s.data(), s.size(), out.data()) == FHS_OK);
        CHECK(fhs_str_compare(c, s.data(), s.size(), s.data(), s.size() - 3, 1, &r) == FHS_OK);   // le: the longer buffer has a non-NUL tail
        CHECK(fhs_trivial_value(c, r, &triv, &val) == FHS_OK && triv == 1 && val == 0);
        CHECK(fhs_flush(c) == FHS_OK);
    }
    {   // a public-key upload on the planner: handles only, nothing is read
        std::vector<uint32_t> m32(2 * 2048, 0), b32(4 * 600, 0);
        std::vector<fhs_char_t> hs(600);
        CHECK(fhs_upload_string_public(c, m32.data(), b32.data(), 600, 0, 600, hs.data()) == FHS_OK);
        CHECK(fhs_upload_string_public(c, m32.data(), b32.data(), 600, 590, 11, hs.data()) == FHS_ERR_ARG);
        uint64_t c2 = 0;
        CHECK(fhs_char_sum_c2(c, hs[599], &c2) == FHS_OK && c2 == 1);
        for (fhs_char_t h : hs) CHECK(fhs_release(c, h) == FHS_OK);
    }
    {   // the string store's host side on the planner: entry table, windows, meta words, one entry left to the context
        std::vector<uint32_t> m32(2 * 2048, 0), b32(4 * 600, 0);
        std::vector<uint64_t> meta(4 * 600, 1 | 3ull << 16 | 2ull << 32);
        std::vector<fhs_char_t> hs(600);
        uint64_t id = 0, id2 = 0, c2 = 0;
        size_t n = 0, bytes = 0;
        CHECK(fhs_store_import(c, m32.data(), b32.data(), meta.data(), 600, &id) == FHS_OK && id != 0);
        meta[2399] = 0;
        CHECK(fhs_store_import(c, m32.data(), b32.data(), meta.data(), 600, &id2) == FHS_ERR_ARG && id2 == 0);
        CHECK(fhs_store_info(c, id, &n, &bytes) == FHS_OK && n == 600 && bytes == 2 * 8192 + 16 * 600);
        CHECK(fhs_store_get(c, id, 590, 11, hs.data()) == FHS_ERR_ARG);
        CHECK(fhs_store_get(c, id, 0, 600, hs.data()) == FHS_OK);
        CHECK(fhs_store_put(c, hs.data(), 600, &id2) == FHS_OK && id2 != id && id2 != 0);
        CHECK(fhs_store_drop(c, id) == FHS_OK && fhs_store_drop(c, id) == FHS_ERR_ARG);
        for (fhs_char_t h : hs) CHECK(fhs_release(c, h) == FHS_OK);
        CHECK(fhs_store_get(c, id2, 599, 1, hs.data()) == FHS_OK);
        CHECK(fhs_char_sum_c2(c, hs[0], &c2) == FHS_OK && c2 == 1);
        CHECK(fhs_release(c, hs[0]) == FHS_OK);
        CHECK(fhs_store_stats(c, &n, nullptr, &bytes) == FHS_OK && n == 1 && bytes == 2 * 8192 + 16 * 600);
        // select by encrypted index on the planner: 600 characters in rows of 8 (75 rows, 7 bits), bookkeeping only
        std::vector<uint64_t> q(FHS_SELECT_QUERY_WORDS(7), 0);
        uint64_t sel = 0;
        uint32_t nk = 0;
        CHECK(fhs_store_select(c, id2, 8, q.data(), 7, &sel) == FHS_OK && sel != 0 && sel != id2);
        CHECK(fhs_store_info(c, sel, &n, &bytes) == FHS_OK && n == 8 && bytes == 8192 + 16 * 8);
        CHECK(fhs_store_rekey_count(c, sel, &nk) == FHS_OK && nk == FHS_SELECT_REKEY_COST * 7);
        CHECK(fhs_store_select(c, id2, 8, q.data(), 6, &sel) == FHS_ERR_ARG && sel == 0);
        CHECK(fhs_store_select(c, id2, 7, q.data(), 7, &sel) == FHS_ERR_ARG && fhs_store_select(c, id2, 8, nullptr, 7, &sel) == FHS_ERR_ARG);
    }
    for (int r = 0; r < 2; r++) {
        // a compressed upload on the planner (handles only), then the all-at-once plan walked as rank r of 2 would:
        // fhs_flush_plan builds whole levels with the level builder of every flush, level_exec counts this rank's slice
        CHECK(fhs_set_mode(c, 1) == FHS_OK && fhs_dist_config(c, r, 2) == FHS_OK);
        const uint32_t seed[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        std::vector<uint64_t> bodies(4 * 40, 0);
        std::vector<fhs_char_t> s(40);
        CHECK(fhs_upload_string_compressed(c, seed, bodies.data(), 40, 3, s.data()) == FHS_OK);
        auto p = dummy(c, 3), to = dummy(c, 2);
        size_t len = 0;
        std::vector<fhs_char_t> rep(fhs_str_replace_len(s.size(), p.size(), to.size()) + 8);
        CHECK(fhs_str_replace(c, s.data(), s.size(), p.data(), p.size(), to.data(), to.size(), rep.data(), rep.size(), &len) == FHS_OK);
        CHECK(fhs_flush(c) == FHS_ERR_STATE);                    // a distributed context is run level by level
        uint64_t n_levels = 0, max_w = 0, slice[1] = {0}, covered = 0;
        CHECK(fhs_flush_plan(c, &n_levels, &max_w) == FHS_OK && n_levels > 5 && max_w > 0);
        fhs_stats before, after;
        CHECK(fhs_get_stats(c, &before) == FHS_OK);
        CHECK(fhs_pool_trim(c, FHS_TRIM_COMPACT, 0, nullptr, nullptr) == FHS_ERR_STATE);   // planned levels are waiting
        for (uint64_t k = 0; k < n_levels; k++) {
            uint64_t width = 0, cap = 0;
            CHECK(fhs_flush_level_exec(c, k, slice, &width, &cap) == FHS_OK && width <= max_w && cap == (width + 1) / 2);
            covered += width > (uint64_t)r * cap ? std::min(cap, width - (uint64_t)r * cap) : 0;
            CHECK(fhs_flush_level_commit(c, k, slice) == FHS_OK);
        }
        CHECK(fhs_get_stats(c, &after) == FHS_OK && after.pbs_executed - before.pbs_executed == covered &&
              after.levels - before.levels == n_levels);
        CHECK(fhs_flush_level_exec(c, 0, slice, &max_w, &max_w) == FHS_ERR_ARG);   // the plan is used up
        CHECK(fhs_dist_config(c, 0, 1) == FHS_OK && fhs_flush(c) == FHS_OK);
        for (fhs_char_t h : s) CHECK(fhs_release(c, h) == FHS_OK);
    }
    fhs_stats st;
    // (mostly plaintext strings: counts over repeated flags may pass the budget slightly, tests/test_planner.py)
    CHECK(fhs_get_stats(c, &st) == FHS_OK && st.pbs_executed > 1000 && st.max_input_sum_c2 <= 160);
    size_t w0, w1, c0, c1;
    fhs_dist_plan_windows(257, 4, 8, 7, &w0, &w1, &c0, &c1);
    CHECK(w1 == 254 && c1 == 257);
    CHECK(fhs_str_find(c, nullptr, 3, nullptr, 0, nullptr) != FHS_OK);   // argument errors do not crash
    {   // block pool: a planner holds no chunk and trims nothing; the victim choice on the host
        uint64_t ps[6] = {9, 9, 9, 9, 9, 9}, moved = 9, released = 9;
        CHECK(fhs_pool_stats(c, ps) == FHS_OK && ps[0] == 0 && ps[1] == 2048 && ps[2] == st.blocks_live && ps[3] == 0 &&
              ps[4] == 0 && ps[5] == 0);
        CHECK(fhs_pool_trim(c, FHS_TRIM_COMPACT, 0, &moved, &released) == FHS_OK && moved == 0 && released == 0);
        CHECK(fhs_pool_trim(c, FHS_TRIM_RELEASE, 7, nullptr, nullptr) == FHS_OK && fhs_pool_trim(c, 2, 0, nullptr, nullptr) == FHS_ERR_ARG);
        const uint32_t live[4] = {2048, 1, 0, 7}, over[1] = {2049};
        uint8_t victim[4] = {9, 9, 9, 9};
        CHECK(fhs_debug_pool_plan(live, 4, 0, victim) == FHS_OK && !victim[0] && victim[1] && victim[2] && !victim[3]);
        CHECK(fhs_debug_pool_plan(live, 4, ~(size_t)0, victim) == FHS_OK && !victim[1] && !victim[2]);
        CHECK(fhs_debug_pool_plan(over, 1, 0, victim) == FHS_ERR_ARG && fhs_debug_pool_plan(nullptr, 0, 0, nullptr) == FHS_OK);
    }
    fhs_ctx_destroy(c);
    {   // a planner destroyed with work outstanding: submitted but unpumped jobs, one store entry, live char handles --
        // nothing is released by hand, every owner and container goes with the context (the leak checker watches)
        fhs_ctx *d = nullptr;
        CHECK(fhs_ctx_create_planner(&d) == FHS_OK && fhs_set_mode(d, 1) == FHS_OK);
        auto s = dummy(d, 20);
        std::vector<fhs_char_t> up(s.size());
        uint64_t id = 0;
        CHECK(fhs_str_to_upper(d, s.data(), s.size(), up.data()) == FHS_OK && fhs_submit(d) == FHS_OK);
        CHECK(fhs_store_put(d, s.data(), s.size(), &id) == FHS_OK && id != 0);
        fhs_char_t r = 0;
        CHECK(fhs_str_contains_clear(d, up.data(), up.size(), "ab", 2, &r) == FHS_OK && fhs_submit(d) == FHS_OK);
        fhs_ctx_destroy(d);
    }
    {   // user tables and the clear maps built on them: registry, the digit plans, both modes
        fhs_ctx *d = nullptr;
        CHECK(fhs_ctx_create_planner(&d) == FHS_OK && fhs_set_mode(d, 1) == FHS_OK);
        uint8_t values[16], table[256], set32[32] = {0};
        for (int v = 0; v < 16; v++) values[v] = (uint8_t)((v * 11 + 5) & 31);
        int id = -1, again = -1;
        const int count0 = fhs_user_lut_count();
        CHECK(fhs_user_lut(values, &id) == FHS_OK && id >= fhs_lut_catalogue_count() && fhs_user_lut(values, &again) == FHS_OK &&
              again == id && fhs_user_lut_count() == count0 + 1);
        values[7] = 32;
        CHECK(fhs_user_lut(values, &again) == FHS_ERR_ARG && fhs_user_lut(nullptr, &again) == FHS_ERR_ARG);
        std::vector<uint64_t> poly(2048);
        CHECK(fhs_debug_lut_poly(id, poly.data()) == FHS_OK && poly[0] == ((uint64_t)5 << 59) && poly[2047] == (uint64_t)0 - ((uint64_t)5 << 59));
        CHECK(fhs_debug_lut_poly(fhs_lut_catalogue_count() + fhs_user_lut_count(), poly.data()) == FHS_ERR_ARG);
        CHECK(fhs_debug_read_lut(d, id, poly.data()) == FHS_ERR_STATE);
        auto s = dummy(d, 9);
        std::vector<fhs_char_t> out(s.size());
        fhs_char_t pos = 0, lo = 0, hi = 0;
        for (int kind = 0; kind < 4; kind++) {               // a case fold, a permutation, every byte anywhere, few rows
            for (int v = 0; v < 256; v++)
                table[v] = (uint8_t)(kind == 0 ? (v >= 'a' && v <= 'z' ? v - 32 : v) : kind == 1 ? (v * 7 + 3) & 255
                                   : kind == 2 ? (v * v * 31 + v / 3) & 255 : ((v >> 6) * 4 + (v & 3)) * 17);
            CHECK(fhs_str_map_clear(d, s.data(), s.size(), table, out.data()) == FHS_OK);
            for (fhs_char_t h : out) CHECK(fhs_release(d, h) == FHS_OK);
        }
        for (int v = 0; v < 256; v++)
            if ((v * 37 + (v >> 3)) % 5 < 2) set32[v >> 3] |= (uint8_t)(1 << (v & 7));
        CHECK(fhs_str_class_flags(d, s.data(), s.size(), set32, out.data()) == FHS_OK);
        CHECK(fhs_str_find_class(d, s.data(), s.size(), set32, &pos) == FHS_OK);
        CHECK(fhs_str_find_class_wide(d, s.data(), s.size(), set32, &lo, &hi) == FHS_OK && fhs_flush(d) == FHS_OK);
        CHECK(fhs_str_map_clear(d, s.data(), s.size(), nullptr, out.data()) == FHS_ERR_ARG);
        CHECK(fhs_set_mode(d, 0) == FHS_OK);                 // as written: a sparse table and a sparse set on trivial characters
        for (int v = 0; v < 256; v++) table[v] = (uint8_t)v;
        table['a'] = 'b';
        table[0] = '-';
        std::memset(set32, 0, sizeof set32);
        set32['b' >> 3] |= (uint8_t)(1 << ('b' & 7));
        fhs_char_t t2[2] = {fhs_trivial(d, 'a'), fhs_trivial(d, 0)}, m2[2], f2[2];
        int triv = 0;
        uint8_t val = 0;
        CHECK(fhs_str_map_clear(d, t2, 2, table, m2) == FHS_OK && fhs_trivial_value(d, m2[1], &triv, &val) == FHS_OK && triv && val == '-');
        CHECK(fhs_str_class_flags(d, m2, 2, set32, f2) == FHS_OK && fhs_trivial_value(d, f2[0], &triv, &val) == FHS_OK && triv && val == 1);
        CHECK(fhs_str_find_class(d, m2, 2, set32, &pos) == FHS_OK && fhs_trivial_value(d, pos, &triv, &val) == FHS_OK && triv && val == 0);
        fhs_ctx_destroy(d);
    }
    {   // no device here: creation fails, the half-built object carries the error text and is destroyed like any other
        fhs_ctx *d = nullptr;
        CHECK(fhs_ctx_create(9999, &d) != FHS_OK && d != nullptr && std::strlen(fhs_last_error(d)) > 10);
        fhs_ctx_destroy(d);
        fhs_ctx_destroy(nullptr);
    }
    // every owner is gone, and the planners and the failed creation acquired nothing
    CHECK(fhs_debug_live_resources(res1) == FHS_OK);
    for (int k = 0; k < 4; k++) CHECK(res1[k] == 0);
    CHECK(res1[4] == res0[4]);
    fhs_client_destroy(ck);
    fhs_client_destroy(ck2);
    std::printf(fails ? "FAILED\n" : "host sanitizer run ok\n");
    return fails ? 1 : 0;
}
