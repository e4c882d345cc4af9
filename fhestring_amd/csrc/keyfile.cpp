#include "keyfile.h"

#include <algorithm>
#include <cstring>

#include "../../include/fhestring_hip.h"
#include "pbs_kernels.h"

namespace fhs {

KeyFileHeader make_header(uint64_t kind) {
    KeyFileHeader h{};
    std::memcpy(h.magic, "FHSKEY01", 8);
    h.kind = kind; h.lwe_n = LWE_N; h.poly_n = POLY_N; h.ks_levels = KS_LEVEL; h.ks_base_log = KS_BASE_LOG;
    h.pbs_base_log = PBS_BASE_LOG; h.bsk_quant_bits = BSK_QUANT_BITS;
    return h;
}
bool header_ok(const KeyFileHeader &h) {
    const KeyFileHeader w = make_header(h.kind);
    return std::memcmp(&h, &w, sizeof(h)) == 0 && h.kind >= 1 && h.kind <= 7;
}

KeyFileWriter::KeyFileWriter(const char *path, uint64_t kind) : f_(std::fopen(path, "wb")), ok_(f_ != nullptr) {
    const KeyFileHeader h = make_header(kind);
    put(&h, sizeof(h));
}
KeyFileWriter &KeyFileWriter::put(const void *p, size_t bytes) {
    ok_ = ok_ && std::fwrite(p, 1, bytes, f_) == bytes;
    return *this;
}
int KeyFileWriter::close() {
    if (f_) ok_ = (std::fclose(f_) == 0) && ok_;
    f_ = nullptr;
    return ok_ ? FHS_OK : FHS_ERR_STATE;
}

KeyFileReader::KeyFileReader(const char *path, std::initializer_list<uint64_t> kinds)
    : f_(std::fopen(path, "rb")), ok_(f_ != nullptr) {
    KeyFileHeader h;
    get(&h, sizeof(h));
    ok_ = ok_ && header_ok(h) && std::find(kinds.begin(), kinds.end(), h.kind) != kinds.end();
    if (ok_) kind_ = h.kind;
}
KeyFileReader &KeyFileReader::get(void *p, size_t bytes) {
    ok_ = ok_ && std::fread(p, 1, bytes, f_) == bytes;
    return *this;
}
KeyFileReader &KeyFileReader::get(std::vector<uint64_t> &v, size_t words) {
    if (ok_) v.resize(words);
    return get(v.data(), words * 8);
}
KeyFileReader &KeyFileReader::skip(size_t bytes) {
    ok_ = ok_ && std::fseek(f_, (long)bytes, SEEK_CUR) == 0;
    return *this;
}
int KeyFileReader::finish(bool require_eof) {
    if (f_) {
        ok_ = ok_ && (!require_eof || std::fgetc(f_) == EOF);
        std::fclose(f_);
        f_ = nullptr;
    }
    return ok_ ? FHS_OK : FHS_ERR_STATE;
}

}  // namespace fhs

using namespace fhs;

// the server-key part of a kind 1 or kind 2 file; what follows the keyswitching key is not looked at
int fhs_read_server_key_file(const char *path, std::vector<uint64_t> &bsk, std::vector<uint64_t> &ksk) {
    KeyFileReader r(path, {1, 2});
    if (r.kind() == 1) r.skip(8 + (LWE_N + POLY_N) * 8);   // seed, lwe_sk, glwe_sk
    return r.get(bsk, (size_t)LWE_N * 4 * POLY_N).get(ksk, (size_t)BIG_N * KS_LEVEL * SMALL_CT).finish(false);
}
int fhs_read_multibit_key_file(const char *path, std::vector<uint64_t> &mb) {
    return KeyFileReader(path, {3}).get(mb, FHS_BSK_MB2_WORDS).finish(true);
}
int fhs_read_compressed_server_key_file(const char *path, uint32_t seed[8], std::vector<uint64_t> &bsk_bodies,
                                        std::vector<uint64_t> &ksk_bodies) {
    return KeyFileReader(path, {4}).get(seed, 32).get(bsk_bodies, FHS_CBSK_BODY_WORDS).get(ksk_bodies, FHS_CKSK_BODY_WORDS)
        .finish(true);
}
int fhs_read_packing_key_file(const char *path, std::vector<uint64_t> &key) {
    return KeyFileReader(path, {5}).get(key, FHS_PACK_KEY_WORDS).finish(true);
}
int fhs_read_public_key_file(const char *path, uint32_t seed[8], std::vector<uint64_t> &body) {
    return KeyFileReader(path, {6}).get(seed, 32).get(body, POLY_N).finish(true);
}
int fhs_read_rekey_key_file(const char *path, std::vector<uint64_t> &key) {
    return KeyFileReader(path, {7}).get(key, FHS_REKEY_KEY_WORDS).finish(true);
}
