// Key files (include/fhestring_hip.h, "key files"): a 64-byte header that names the kind and the parameter set, then raw
// little-endian arrays.  One writer and one reader for the seven kinds:
//   1 client key (seed, both secret keys, bsk, ksk)   2 server key (bsk, ksk)   3 pair key   4 compressed server key
//   5 packing key   6 public key   7 re-key key of the string store
#pragma once
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

namespace fhs {

constexpr int PBS_BASE_LOG = 23;   // one GGSW level of base 2^23 (the header records it; the kernels have it built in)

struct KeyFileHeader {
    char magic[8];
    uint64_t kind, lwe_n, poly_n, ks_levels, ks_base_log, pbs_base_log, bsk_quant_bits;
};
static_assert(sizeof(KeyFileHeader) == 64, "header is 64 bytes");
KeyFileHeader make_header(uint64_t kind);
bool header_ok(const KeyFileHeader &h);   // magic, this build's parameters, kind 1..7

// Opens `path` and writes the header of `kind`; put() appends; close() is FHS_OK when every step succeeded, FHS_ERR_STATE
// otherwise (the open included).  The file is closed on every path.
class KeyFileWriter {
public:
    KeyFileWriter(const char *path, uint64_t kind);
    ~KeyFileWriter() { close(); }
    KeyFileWriter(const KeyFileWriter &) = delete;
    KeyFileWriter &operator=(const KeyFileWriter &) = delete;
    KeyFileWriter &put(const void *p, size_t bytes);
    int close();

private:
    FILE *f_;
    bool ok_;
};

// Opens `path` and accepts a valid header whose kind is one of `kinds`.  After the first failure every further step
// does nothing, and finish() reports it.
class KeyFileReader {
public:
    KeyFileReader(const char *path, std::initializer_list<uint64_t> kinds);
    ~KeyFileReader() { finish(false); }
    KeyFileReader(const KeyFileReader &) = delete;
    KeyFileReader &operator=(const KeyFileReader &) = delete;
    uint64_t kind() const { return kind_; }   // 0: no acceptable header
    KeyFileReader &get(void *p, size_t bytes);
    KeyFileReader &get(std::vector<uint64_t> &v, size_t words);   // sizes v, then reads it
    KeyFileReader &skip(size_t bytes);
    // FHS_OK / FHS_ERR_STATE; require_eof: a byte after the last one read is a failure
    int finish(bool require_eof);

private:
    FILE *f_;
    bool ok_;
    uint64_t kind_ = 0;
};

}  // namespace fhs

// The readers behind the fhs_*_file entry points: FHS_OK or FHS_ERR_STATE (missing, truncated, another kind, other
// parameters).  Kinds 3 to 7 must end where their arrays end; the readers of kinds 1 and 2 (this one and
// fhs_client_load) accept trailing bytes.  That difference is as found, pinned by tests/test_client_kat.py, not a rule.
int fhs_read_server_key_file(const char *path, std::vector<uint64_t> &bsk, std::vector<uint64_t> &ksk);   // kinds 1, 2
int fhs_read_multibit_key_file(const char *path, std::vector<uint64_t> &mb);                               // kind 3
int fhs_read_compressed_server_key_file(const char *path, uint32_t seed[8], std::vector<uint64_t> &bsk_bodies,
                                        std::vector<uint64_t> &ksk_bodies);                                // kind 4
int fhs_read_packing_key_file(const char *path, std::vector<uint64_t> &key);                               // kind 5
int fhs_read_public_key_file(const char *path, uint32_t seed[8], std::vector<uint64_t> &body);             // kind 6
int fhs_read_rekey_key_file(const char *path, std::vector<uint64_t> &key);                                 // kind 7
