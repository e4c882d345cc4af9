// extern "C" boundary, part 2: FheAsciiChar ops, MyServerKey string methods, statistics.
#include <algorithm>

#include "capi_internal.h"
#include "keyfile.h"

using namespace fhs;

namespace {

FChar load(Engine &e, fhs_char_t h) {
    FChar c;
    const Bid *b = e.char_blocks(h);
    for (int i = 0; i < 4; i++) {
        e.retain(b[i]);
        c.b[i] = Ref(&e, b[i]);
        // results handed back as sums of bootstrap outputs (find's index digits: up to 57 variances) are refreshed when
        // they come back in as operands; verdict-like sums (<= 4) pass, every operator budgets for those
        if (e.sum_c2(b[i]) > 4) c.b[i] = pbs(c.b[i], LUT_MSG);
    }
    return c;
}
fhs_char_t store(Engine &e, FChar &c) {
    Bid b[4];
    for (int i = 0; i < 4; i++) b[i] = c.b[i].detach();
    return e.new_char(b);
}
bool ok(fhs_ctx *c, fhs_char_t h) { return c && c->eng.valid_char(h); }
bool ok_all(fhs_ctx *c, const fhs_char_t *h, size_t n) {
    if (!c || (n && !h)) return false;
    for (size_t i = 0; i < n; i++)
        if (!c->eng.valid_char(h[i])) return false;
    return true;
}
FStr load_str(Engine &e, const fhs_char_t *h, size_t n) {
    FStr s;
    s.reserve(n);
    for (size_t i = 0; i < n; i++) s.push_back(load(e, h[i]));
    return s;
}
struct PosArg {                                              // a position operand: {{pos}, 1} or {{lo, hi}, 2}
    fhs_char_t h[2];
    size_t halves;
};
bool ok_pos(fhs_ctx *c, const PosArg &p) { return ok_all(c, p.h, p.halves); }
Pos load_pos(fhs_ctx *c, const PosArg &p) { return load_str(c->eng, p.h, p.halves); }
void store_str(Engine &e, FStr &s, fhs_char_t *out) {
    for (size_t i = 0; i < s.size(); i++) out[i] = store(e, s[i]);
}
int bad(fhs_ctx *c) { return c ? c->eng.ctx.fail(FHS_ERR_ARG, "invalid handle or null argument") : FHS_ERR_ARG; }
// the blocks behind n char handles, in order; fails on the first handle that is not valid
int gather_blocks(fhs_ctx *c, const fhs_char_t *chars, size_t n, std::vector<Bid> &out) {
    out.resize(4 * n);
    for (size_t i = 0; i < n; i++) {
        if (!c->eng.valid_char(chars[i])) return bad(c);
        std::copy_n(c->eng.char_blocks(chars[i]), 4, &out[4 * i]);
    }
    return FHS_OK;
}

template <class F> fhs_char_t binop(fhs_ctx *c, fhs_char_t a, fhs_char_t b, F f) {
    if (!ok(c, a) || !ok(c, b)) { bad(c); return 0; }
    FChar r = f(load(c->eng, a), load(c->eng, b));
    return store(c->eng, r);
}
template <class F> fhs_char_t unop(fhs_ctx *c, fhs_char_t a, F f) {
    if (!ok(c, a)) { bad(c); return 0; }
    FChar r = f(load(c->eng, a));
    return store(c->eng, r);
}
int finish(fhs_ctx *c, Strings &S) {
    if (S.err.code) return c->eng.ctx.fail(S.err.code, S.err.msg);
    return FHS_OK;
}

}  // namespace

extern "C" {

fhs_char_t fhs_trivial(fhs_ctx *c, uint8_t v) {
    if (!c) return 0;
    FChar r = ch_trivial(&c->eng, v);
    return store(c->eng, r);
}
fhs_char_t fhs_upload(fhs_ctx *c, const uint64_t *blocks) {
    fhs_char_t h = 0;
    return fhs_upload_string(c, blocks, 1, &h) == FHS_OK ? h : 0;
}
int fhs_upload_string(fhs_ctx *c, const uint64_t *blocks, size_t n, fhs_char_t *out) {
    if (!c || (n && (!blocks || !out))) return bad(c);
    if (!c->eng.planner && hipSetDevice(c->eng.ctx.device) != hipSuccess) return c->eng.ctx.fail(FHS_ERR_HIP, "hipSetDevice failed");
    std::vector<Bid> b(4 * n);
    if (c->eng.from_host_many(blocks, 4 * n, b.data())) return c->eng.ctx.fail(FHS_ERR_HIP, "upload failed (device allocation or copy)");
    for (size_t i = 0; i < n; i++) out[i] = c->eng.new_char(&b[4 * i]);
    return FHS_OK;
}
int fhs_upload_string_compressed(fhs_ctx *c, const uint32_t seed[8], const uint64_t *bodies, size_t n, size_t first_char,
                                 fhs_char_t *out) {
    if (!c || !seed || (n && (!bodies || !out)) || first_char > ((size_t)1 << 60) || n > ((size_t)1 << 60)) return bad(c);
    if (!c->eng.planner && hipSetDevice(c->eng.ctx.device) != hipSuccess) return c->eng.ctx.fail(FHS_ERR_HIP, "hipSetDevice failed");
    std::vector<Bid> b(4 * n);
    if (c->eng.from_compressed_many(seed, bodies, 4 * n, 4 * (uint64_t)first_char, b.data()))
        return c->eng.ctx.fail(FHS_ERR_HIP, "compressed upload failed (device allocation, copy or expansion launch)");
    for (size_t i = 0; i < n; i++) out[i] = c->eng.new_char(&b[4 * i]);
    return FHS_OK;
}
int fhs_upload_string_public(fhs_ctx *c, const void *mask32, const void *body32, size_t n_total, size_t first_char,
                             size_t count, fhs_char_t *out) {
    if (!c || n_total > ((size_t)1 << 24) || first_char > n_total || count > n_total - first_char ||
        (count && (!mask32 || !body32 || !out)))
        return bad(c);
    if (!c->eng.planner && hipSetDevice(c->eng.ctx.device) != hipSuccess) return c->eng.ctx.fail(FHS_ERR_HIP, "hipSetDevice failed");
    std::vector<Bid> b(4 * count);
    if (c->eng.from_public_many(static_cast<const uint32_t *>(mask32), static_cast<const uint32_t *>(body32), 4 * count,
                                4 * (uint64_t)first_char, b.data()))
        return c->eng.ctx.fail(FHS_ERR_HIP, "public-key upload failed (device allocation, copy or expansion launch)");
    for (size_t i = 0; i < count; i++) out[i] = c->eng.new_char(&b[4 * i]);
    return FHS_OK;
}
fhs_char_t fhs_import_device(fhs_ctx *c, const uint64_t *d_blocks) {
    if (!c || !d_blocks) { bad(c); return 0; }
    Bid b[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        b[i] = c->eng.from_device(d_blocks + (size_t)i * FHS_BIG_CT);
        if (!b[i]) {
            for (int k = 0; k < i; k++) c->eng.release(b[k]);
            c->eng.ctx.fail(FHS_ERR_HIP, "import failed");
            return 0;
        }
    }
    return c->eng.new_char(b);
}
fhs_char_t fhs_eq(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_eq); }
fhs_char_t fhs_ne(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_ne); }
fhs_char_t fhs_le(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_le); }
fhs_char_t fhs_lt(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_lt); }
fhs_char_t fhs_ge(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_ge); }
fhs_char_t fhs_gt(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_gt); }
fhs_char_t fhs_bitand(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_bitand); }
fhs_char_t fhs_bitor(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_bitor); }
fhs_char_t fhs_sub(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_sub); }
fhs_char_t fhs_add(fhs_ctx *c, fhs_char_t a, fhs_char_t b) { return binop(c, a, b, ch_add); }
fhs_char_t fhs_if_then_else(fhs_ctx *c, fhs_char_t cond, fhs_char_t t, fhs_char_t f) {
    if (!ok(c, cond) || !ok(c, t) || !ok(c, f)) { bad(c); return 0; }
    FChar r = ch_ite(load(c->eng, cond), load(c->eng, t), load(c->eng, f));
    return store(c->eng, r);
}
fhs_char_t fhs_flip(fhs_ctx *c, fhs_char_t a) { return unop(c, a, ch_flip); }
fhs_char_t fhs_is_whitespace(fhs_ctx *c, fhs_char_t a) { return unop(c, a, ch_is_whitespace); }
fhs_char_t fhs_is_uppercase(fhs_ctx *c, fhs_char_t a) { return unop(c, a, ch_is_uppercase); }
fhs_char_t fhs_is_lowercase(fhs_ctx *c, fhs_char_t a) { return unop(c, a, ch_is_lowercase); }
fhs_char_t fhs_clone(fhs_ctx *c, fhs_char_t a) {
    if (!ok(c, a)) { bad(c); return 0; }
    FChar r = load(c->eng, a);
    return store(c->eng, r);
}
int fhs_release(fhs_ctx *c, fhs_char_t a) {
    if (!ok(c, a)) return bad(c);
    c->eng.free_char(a);
    return FHS_OK;
}
int fhs_flush(fhs_ctx *c) {
    if (!c) return FHS_ERR_ARG;
    int rc = c->eng.flush();
    if (rc) return rc;
    if (c->eng.planner) return FHS_OK;
    if (hipStreamSynchronize(c->eng.ctx.stream) != hipSuccess) return c->eng.ctx.fail(FHS_ERR_HIP, "stream sync failed");
    return FHS_OK;
}
int fhs_set_auto_flush(fhs_ctx *c, size_t n_pending) {
    if (!c) return FHS_ERR_ARG;
    c->eng.auto_flush_pending = n_pending;
    return FHS_OK;
}
int fhs_set_tick_balance(fhs_ctx *c, size_t slots) {
    if (!c) return FHS_ERR_ARG;
    c->eng.balance_slots = slots;
    return FHS_OK;
}
int fhs_resident_slots(const fhs_ctx *c) {
    if (!c) return FHS_ERR_ARG;
    // ciphertexts the selected blind-rotation kernel works on at a time: 4 workgroups of 2 wavefronts per CU for the
    // f64-FFT kernels (persistent), 2 workgroups of 4 wavefronts per CU for the exact ones
    return fhs::is_f64_fft(c->eng.ctx.arith) ? c->eng.ctx.wg_slots : c->eng.ctx.wg_slots / 2;
}

int fhs_submit(fhs_ctx *c) {
    if (!c) return FHS_ERR_ARG;
    return c->eng.submit();
}
int fhs_pump(fhs_ctx *c, size_t n_ticks) {
    if (!c) return FHS_ERR_ARG;
    return c->eng.pump(n_ticks);
}
int fhs_flush_async(fhs_ctx *c) {
    if (!c) return FHS_ERR_ARG;
    return c->eng.flush();
}
int fhs_download(fhs_ctx *c, fhs_char_t a, uint64_t *blocks) {
    if (!ok(c, a) || !blocks) return bad(c);
    const Bid *b = c->eng.char_blocks(a);
    for (int i = 0; i < 4; i++) {
        int rc = c->eng.read_block(b[i], blocks + (size_t)i * FHS_BIG_CT);
        if (rc) return rc;
    }
    return FHS_OK;
}
int fhs_download_string(fhs_ctx *c, const fhs_char_t *chars, size_t n, uint64_t *blocks) {
    if (!c || (n && (!chars || !blocks))) return bad(c);
    std::vector<Bid> b;
    if (int rc = gather_blocks(c, chars, n, b)) return rc;
    return c->eng.read_many(b.data(), b.size(), blocks);
}
int fhs_load_packing_key(fhs_ctx *c, const uint64_t *key) {
    if (!c) return FHS_ERR_ARG;
    if (c->eng.planner) return FHS_OK;                       // like fhs_load_multibit_key: a planner holds no key
    if (int rc = c->eng.flush()) return rc;
    return c->eng.ctx.load_packing_key(key);
}
namespace {
int download_packed(fhs_ctx *c, const fhs_char_t *chars, size_t n, void *mask16, void *body16, uint64_t *mask64,
                    uint64_t *body64, bool recipient) {
    if (!c || (n && (!chars || !mask16 || !body16)) || !mask64 != !body64) return bad(c);
    if (recipient && n == 0) return FHS_OK;
    std::vector<Bid> b;
    if (int rc = gather_blocks(c, chars, n, b)) return rc;
    return c->eng.read_packed(b.data(), b.size(), static_cast<uint16_t *>(mask16), static_cast<uint16_t *>(body16), mask64,
                              body64, recipient);
}
}  // namespace
int fhs_debug_download_string_packed64(fhs_ctx *c, const fhs_char_t *chars, size_t n, void *mask16, void *body16,
                                       uint64_t *mask64, uint64_t *body64) {
    return download_packed(c, chars, n, mask16, body16, mask64, body64, false);
}
int fhs_download_string_packed(fhs_ctx *c, const fhs_char_t *chars, size_t n, void *mask16, void *body16) {
    return fhs_debug_download_string_packed64(c, chars, n, mask16, body16, nullptr, nullptr);
}

// ---- device-resident string store ----
int fhs_store_put(fhs_ctx *c, const fhs_char_t *chars, size_t n, uint64_t *id_out) {
    if (!c || !id_out || (n && !chars)) return bad(c);
    *id_out = 0;
    std::vector<Bid> b;
    if (int rc = gather_blocks(c, chars, n, b)) return rc;
    return c->eng.store_put(b.data(), b.size(), id_out);
}
int fhs_store_get(fhs_ctx *c, uint64_t id, size_t first_char, size_t count, fhs_char_t *out) {
    if (!c || (count && !out)) return bad(c);
    const Engine::StoreEntry *ent = c->eng.store_entry(id);
    if (!ent) return c->eng.ctx.fail(FHS_ERR_ARG, "string store: unknown entry id");
    const size_t n_chars = ent->n_blocks / 4;
    if (first_char > n_chars || count > n_chars - first_char) return c->eng.ctx.fail(FHS_ERR_ARG, "string store: window outside the entry");
    std::vector<Bid> b(4 * count);
    if (int rc = c->eng.store_get(id, 4 * first_char, 4 * count, b.data())) return rc;
    for (size_t i = 0; i < count; i++) out[i] = c->eng.new_char(&b[4 * i]);
    return FHS_OK;
}
int fhs_store_drop(fhs_ctx *c, uint64_t id) {
    if (!c) return FHS_ERR_ARG;
    return c->eng.store_drop(id);
}
int fhs_store_info(fhs_ctx *c, uint64_t id, size_t *n_chars, size_t *device_bytes) {
    if (!c) return FHS_ERR_ARG;
    const Engine::StoreEntry *ent = c->eng.store_entry(id);
    if (!ent) return c->eng.ctx.fail(FHS_ERR_ARG, "string store: unknown entry id");
    if (n_chars) *n_chars = ent->n_blocks / 4;
    if (device_bytes) *device_bytes = ent->bytes();
    return FHS_OK;
}
int fhs_store_stats(fhs_ctx *c, size_t *entries, size_t *chars, size_t *device_bytes) {
    if (!c) return FHS_ERR_ARG;
    size_t blocks = 0;
    c->eng.store_stats(entries, &blocks, device_bytes);
    if (chars) *chars = blocks / 4;
    return FHS_OK;
}
int fhs_store_export(fhs_ctx *c, uint64_t id, void *mask32, void *body32, uint64_t *meta) {
    if (!c || !mask32 || !body32 || !meta) return bad(c);
    return c->eng.store_export(id, static_cast<uint32_t *>(mask32), static_cast<uint32_t *>(body32), meta);
}
int fhs_store_import(fhs_ctx *c, const void *mask32, const void *body32, const uint64_t *meta, size_t n, uint64_t *id_out) {
    if (!c || !id_out) return bad(c);
    *id_out = 0;
    if (n > ((size_t)1 << 24) || (n && (!mask32 || !body32))) return bad(c);
    return c->eng.store_import(static_cast<const uint32_t *>(mask32), static_cast<const uint32_t *>(body32), meta, 4 * n, id_out);
}
// ---- block pool: accounting and trimming ----
int fhs_pool_stats(fhs_ctx *c, uint64_t out[6]) {
    if (!c || !out) return bad(c);
    c->eng.pool_stats(out);
    return FHS_OK;
}
int fhs_pool_trim(fhs_ctx *c, int mode, size_t keep_free_blocks, uint64_t *blocks_moved, uint64_t *bytes_released) {
    if (!c || (mode != FHS_TRIM_RELEASE && mode != FHS_TRIM_COMPACT)) return bad(c);
    return c->eng.pool_trim(mode == FHS_TRIM_COMPACT, keep_free_blocks, blocks_moved, bytes_released);
}
int fhs_debug_pool_plan(const uint32_t *live_per_chunk, size_t n_chunks, size_t keep_free_blocks, uint8_t *victim_out) {
    if (n_chunks && (!live_per_chunk || !victim_out)) return FHS_ERR_ARG;
    if (n_chunks > ((size_t)1 << 24)) return FHS_ERR_ARG;
    for (size_t i = 0; i < n_chunks; i++)
        if (live_per_chunk[i] > BlockPool::CHUNK_BLOCKS) return FHS_ERR_ARG;
    BlockPool::plan_trim(live_per_chunk, n_chunks, keep_free_blocks, victim_out);
    return FHS_OK;
}
int fhs_load_packing_key_file(fhs_ctx *c, const char *path) {
    if (!c || !path) return FHS_ERR_ARG;
    std::vector<uint64_t> key;
    if (fhs_read_packing_key_file(path, key) != FHS_OK)
        return c->eng.ctx.fail(FHS_ERR_STATE, "cannot read packing key file (missing, truncated, not kind 5 or wrong parameters)");
    return fhs_load_packing_key(c, key.data());
}
// ---- string store: re-key ----
int fhs_load_rekey_key(fhs_ctx *c, const uint64_t *key) {
    if (!c) return FHS_ERR_ARG;
    if (c->eng.planner) {                                    // a planner converts nothing: it notes whether a key is there
        c->eng.planner_rekey_key = key != nullptr;
        return FHS_OK;
    }
    return c->eng.ctx.load_rekey_key(key);
}
int fhs_load_rekey_key_file(fhs_ctx *c, const char *path) {
    if (!c || !path) return FHS_ERR_ARG;
    std::vector<uint64_t> key;
    if (fhs_read_rekey_key_file(path, key) != FHS_OK)
        return c->eng.ctx.fail(FHS_ERR_STATE, "cannot read re-key key file (missing, truncated, not kind 7 or wrong parameters)");
    return fhs_load_rekey_key(c, key.data());
}
int fhs_store_rekey(fhs_ctx *c, uint64_t id, uint64_t *id_out) {
    if (!c) return FHS_ERR_ARG;
    if (id_out) *id_out = 0;
    return c->eng.store_rekey(id, id_out);
}
int fhs_store_rekey_count(fhs_ctx *c, uint64_t id, uint32_t *n) {
    if (!c || !n) return bad(c);
    const Engine::StoreEntry *ent = c->eng.store_entry(id);
    if (!ent) return c->eng.ctx.fail(FHS_ERR_ARG, "string store: unknown entry id");
    *n = ent->rekeys;
    return FHS_OK;
}
int fhs_debug_rekey_device(fhs_ctx *c, const void *mask32, const void *body32, size_t n_blocks, void *mask32_out,
                           void *body32_out) {
    if (!c || (n_blocks && (!mask32 || !body32 || !mask32_out || !body32_out)) || n_blocks > ((size_t)1 << 26)) return bad(c);
    return c->eng.debug_rekey(static_cast<const uint32_t *>(mask32), static_cast<const uint32_t *>(body32), n_blocks,
                              static_cast<uint32_t *>(mask32_out), static_cast<uint32_t *>(body32_out));
}
// ---- string store: select by encrypted index ----
namespace {
using SelectQueries = Engine::SelectQueries;
// what fhs_store_select_batch refuses before the engine sees it: a form, a count or a pointer
bool batch_args_ok(int form, const uint32_t *seeds, const uint64_t *const *queries, size_t n) {
    if (form != FHS_SELECT_FORM_FULL && form != FHS_SELECT_FORM_SEEDED) return false;
    if (!queries || n == 0 || n > (size_t)FHS_SELECT_MAX_BATCH || (form == FHS_SELECT_FORM_SEEDED && !seeds)) return false;
    for (size_t i = 0; i < n; i++)
        if (!queries[i]) return false;
    return true;
}
}  // namespace
int fhs_store_select(fhs_ctx *c, uint64_t id, size_t row_chars, const uint64_t *query, int bits, uint64_t *id_out) {
    if (!c || !id_out) return bad(c);
    *id_out = 0;
    if (!query) return bad(c);
    return c->eng.store_select(id, row_chars, SelectQueries{FHS_SELECT_FORM_FULL, nullptr, &query, 1}, bits, false, id_out);
}
int fhs_store_select_seeded(fhs_ctx *c, uint64_t id, size_t row_chars, const uint32_t seed[8], const uint64_t *bodies, int bits,
                            uint64_t *id_out) {
    if (!c || !id_out) return bad(c);
    *id_out = 0;
    if (!seed || !bodies) return bad(c);
    return c->eng.store_select(id, row_chars, SelectQueries{FHS_SELECT_FORM_SEEDED, seed, &bodies, 1}, bits, false, id_out);
}
int fhs_store_select_batch(fhs_ctx *c, uint64_t id, size_t row_chars, int form, const uint32_t *seeds,
                           const uint64_t *const *queries, size_t n, int bits, uint64_t *ids_out) {
    if (!c || !ids_out) return bad(c);
    for (size_t i = 0; i < n && i < (size_t)FHS_SELECT_MAX_BATCH; i++) ids_out[i] = 0;
    if (!batch_args_ok(form, seeds, queries, n)) return bad(c);
    return c->eng.store_select(id, row_chars, SelectQueries{form, seeds, queries, n}, bits, true, ids_out);
}
size_t fhs_store_select_batch_bytes(size_t n_chars, size_t row_chars, size_t n) {
    return Engine::select_batch_bytes(n_chars, row_chars, n);
}
int fhs_debug_select_device(fhs_ctx *c, const uint64_t *query, int bits, const void *mask32, const void *body32, size_t n_blocks,
                            size_t row_chars, void *mask32_out, void *body32_out) {
    if (!c || !query || !mask32 || !body32 || !mask32_out || !body32_out) return bad(c);
    return c->eng.debug_select(SelectQueries{FHS_SELECT_FORM_FULL, nullptr, &query, 1}, bits, static_cast<const uint32_t *>(mask32),
                               static_cast<const uint32_t *>(body32), n_blocks, row_chars, static_cast<uint32_t *>(mask32_out),
                               static_cast<uint32_t *>(body32_out));
}
int fhs_debug_select_seeded_device(fhs_ctx *c, const uint32_t seed[8], const uint64_t *bodies, int bits, const void *mask32,
                                   const void *body32, size_t n_blocks, size_t row_chars, void *mask32_out, void *body32_out) {
    if (!c || !seed || !bodies || !mask32 || !body32 || !mask32_out || !body32_out) return bad(c);
    return c->eng.debug_select(SelectQueries{FHS_SELECT_FORM_SEEDED, seed, &bodies, 1}, bits, static_cast<const uint32_t *>(mask32),
                               static_cast<const uint32_t *>(body32), n_blocks, row_chars, static_cast<uint32_t *>(mask32_out),
                               static_cast<uint32_t *>(body32_out));
}
int fhs_debug_select_query_device(fhs_ctx *c, int form, const uint32_t seed[8], const uint64_t *words, int bits, double *out) {
    if (!c || !words || !out || (form != FHS_SELECT_FORM_FULL && form != FHS_SELECT_FORM_SEEDED) ||
        (form == FHS_SELECT_FORM_SEEDED && !seed))
        return bad(c);
    return c->eng.debug_select_query(SelectQueries{form, form == FHS_SELECT_FORM_SEEDED ? seed : nullptr, &words, 1}, bits, out);
}
int fhs_select_query_ntt_host(const uint64_t *query, int bits, double *out) {
    if (!query || !out || bits < 1 || bits > 24) return FHS_ERR_ARG;
    convert_polys_to_ntt(query, out, (size_t)bits * SELECT_BIT_POLYS, BSK_QUANT_BITS);
    return FHS_OK;
}
// ---- packed result download under a recipient's key ----
int fhs_download_string_packed_for(fhs_ctx *c, const fhs_char_t *chars, size_t n, void *mask16, void *body16, uint64_t *mask64,
                                   uint64_t *body64) {
    return download_packed(c, chars, n, mask16, body16, mask64, body64, true);
}
int fhs_debug_rekey_packed_device(fhs_ctx *c, const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, void *mask16,
                                  void *body16) {
    if (!c || (n_blocks && (!mask64 || !body64 || !mask16 || !body16)) || n_blocks > ((size_t)1 << 26)) return bad(c);
    return c->eng.debug_rekey_packed(mask64, body64, n_blocks, static_cast<uint16_t *>(mask16), static_cast<uint16_t *>(body16));
}
// ---- string store: packed download of parked entries ----
int fhs_store_download_packed(fhs_ctx *c, uint64_t id, size_t first_char, size_t count, int recipient, void *mask16, void *body16) {
    if (!c || (count && (!mask16 || !body16))) return bad(c);
    return c->eng.store_read_packed(id, first_char, count, recipient != 0, static_cast<uint16_t *>(mask16),
                                    static_cast<uint16_t *>(body16));
}
namespace {
int export_device(fhs_ctx *c, fhs_char_t a, uint64_t *d_blocks, bool wait) {
    if (!ok(c, a) || !d_blocks) return bad(c);
    const Bid *b = c->eng.char_blocks(a);
    for (int i = 0; i < 4; i++) {
        int rc = c->eng.copy_block_to_device(b[i], d_blocks + (size_t)i * FHS_BIG_CT, wait);
        if (rc) return rc;
    }
    return FHS_OK;
}
}  // namespace
int fhs_export_device(fhs_ctx *c, fhs_char_t a, uint64_t *d_blocks) { return export_device(c, a, d_blocks, true); }
int fhs_export_device_async(fhs_ctx *c, fhs_char_t a, uint64_t *d_blocks) { return export_device(c, a, d_blocks, false); }
void *fhs_stream_handle(fhs_ctx *c) { return c ? static_cast<hipStream_t>(c->eng.ctx.stream) : nullptr; }

int fhs_set_mode(fhs_ctx *c, int mode) {
    if (!c || (mode != FHS_MODE_AS_WRITTEN && mode != FHS_MODE_FUSED)) return bad(c);
    c->eng.mode = mode;
    return FHS_OK;
}

#define STR_PAT_OP(NAME, METHOD)                                                                         \
    int NAME(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out) { \
        if (!ok_all(c, s, n) || !ok_all(c, pat, m) || !out) return bad(c);                               \
        Strings S(&c->eng);                                                                              \
        FChar r = S.METHOD(load_str(c->eng, s, n), load_str(c->eng, pat, m));                            \
        if (int rc = finish(c, S)) return rc;                                                            \
        *out = store(c->eng, r);                                                                         \
        return FHS_OK;                                                                                   \
    }
STR_PAT_OP(fhs_str_contains, contains)
STR_PAT_OP(fhs_str_starts_with, starts_with)
STR_PAT_OP(fhs_str_ends_with, ends_with)
STR_PAT_OP(fhs_str_eq, eq)
STR_PAT_OP(fhs_str_ne, ne)
STR_PAT_OP(fhs_str_eq_ignore_case, eq_ignore_case)

int fhs_str_contains_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, fhs_char_t *out) {
    if (!ok_all(c, s, n) || (m && !pat) || !out) return bad(c);
    Strings S(&c->eng);
    FChar r = S.contains(load_str(c->eng, s, n), S.clear(pat, m));
    *out = store(c->eng, r);
    return FHS_OK;
}
// LIKE against a clear pattern.  The pattern is judged before the string is loaded: loading
// refreshes noisy operands, which records bootstraps.
int fhs_str_like_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, int escape, uint32_t flags,
                       fhs_char_t *out) {
    if (!ok_all(c, s, n) || (m && !pat) || !out) return bad(c);
    if (flags & ~(uint32_t)FHS_LIKE_IGNORE_CASE) return c->eng.ctx.fail(FHS_ERR_ARG, "fhs_str_like_clear: unknown flag bits");
    std::vector<Strings::LikeTok> tok;
    if (!Strings::like_parse(pat, m, escape, &tok))
        return c->eng.ctx.fail(FHS_ERR_ARG, "fhs_str_like_clear: a NUL in the pattern, an escape byte that is 0, '%' or '_', or "
                                            "an escape that is not followed by '%', '_' or itself");
    Strings S(&c->eng);
    const int known = Strings::like_trivial(tok, n);
    FChar r = known >= 0 ? ch_trivial(&c->eng, (uint8_t)known)
                         : S.like(load_str(c->eng, s, n), tok, (flags & FHS_LIKE_IGNORE_CASE) != 0);
    *out = store(c->eng, r);
    return FHS_OK;
}
// A regular expression against a clear pattern.  As with LIKE the pattern is judged, and what it
// decides alone is answered, before the string is loaded; the class tables are registered before that too.
int fhs_regex_info(const char *pat, size_t m, uint32_t flags, size_t *positions, size_t *min_len, size_t *err_offset) {
    if (positions) *positions = 0;
    if (min_len) *min_len = 0;
    if (err_offset) *err_offset = 0;
    if ((m && !pat) || (flags & ~(uint32_t)(FHS_REGEX_IGNORE_CASE | FHS_REGEX_SEARCH))) return FHS_ERR_ARG;
    RegexProgram g;
    const RegexStatus st = regex_compile(pat, m, (flags & FHS_REGEX_IGNORE_CASE) != 0, (flags & FHS_REGEX_SEARCH) != 0, &g,
                                         err_offset, nullptr);
    if (st != REGEX_OK) return st == REGEX_LIMIT ? FHS_ERR_LIMIT : FHS_ERR_ARG;
    if (positions) *positions = g.positions();
    if (min_len) *min_len = g.min_len;
    return FHS_OK;
}
int fhs_str_regex_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags, fhs_char_t *out) {
    if (!ok_all(c, s, n) || (m && !pat) || !out) return bad(c);
    if (flags & ~(uint32_t)(FHS_REGEX_IGNORE_CASE | FHS_REGEX_SEARCH))
        return c->eng.ctx.fail(FHS_ERR_ARG, "fhs_str_regex_clear: unknown flag bits");
    RegexProgram g;
    const char *why = "";
    const RegexStatus st = regex_compile(pat, m, (flags & FHS_REGEX_IGNORE_CASE) != 0, (flags & FHS_REGEX_SEARCH) != 0, &g,
                                         nullptr, &why);
    if (st != REGEX_OK) return c->eng.ctx.fail(st == REGEX_LIMIT ? FHS_ERR_LIMIT : FHS_ERR_ARG, why);
    Strings S(&c->eng);
    const int known = Strings::regex_trivial(g, n);
    FChar r;
    if (known >= 0) r = ch_trivial(&c->eng, (uint8_t)known);
    else {
        Strings::RegexPlan plan;
        if (!S.regex_plan(g, &plan)) return finish(c, S);
        r = S.regex(load_str(c->eng, s, n), g, plan);
        if (int rc = finish(c, S)) return rc;
    }
    *out = store(c->eng, r);
    return FHS_OK;
}
// Where a match starts: the flags of all starts (`flags`), or the first start as a position (lo,
// hi).  The order of fhs_str_regex_clear: the pattern, what it decides alone, the tables, and only then the string.
namespace {
int regex_find_op(fhs_ctx *c, const char *name, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags,
                  fhs_char_t *starts, fhs_char_t *lo, fhs_char_t *hi) {
    if (flags & ~(uint32_t)FHS_REGEX_IGNORE_CASE)
        return c->eng.ctx.fail(FHS_ERR_ARG, std::string(name) + ": FHS_REGEX_IGNORE_CASE is the only flag bit these calls take");
    RegexProgram g;
    const char *why = "";
    const RegexStatus st = regex_compile(pat, m, (flags & FHS_REGEX_IGNORE_CASE) != 0, false, &g, nullptr, &why);
    if (st != REGEX_OK) return c->eng.ctx.fail(st == REGEX_LIMIT ? FHS_ERR_LIMIT : FHS_ERR_ARG, why);
    const size_t halves = hi ? 2 : 1;
    if (lo && n > ((size_t)1 << (8 * halves))) return c->eng.ctx.fail(FHS_ERR_LIMIT, Strings::LIMIT_MSG);
    const RegexProgram rev = regex_reverse(g);
    Strings S(&c->eng);
    Strings::RegexPlan plan;
    // decided by the pattern alone: the string is not loaded, the empty one gives the same position; the start flags of
    // a nullable pattern are "no NUL before i", which the string decides
    const int known = Strings::regex_find_trivial(rev, n);
    const bool decided = known == 0 || (known == 1 && !starts);
    if (!decided && !S.regex_plan(rev, &plan)) return finish(c, S);
    const FStr text = decided ? FStr() : load_str(c->eng, s, n);
    if (starts) {
        FStr r = decided ? FStr(n, ch_trivial(&c->eng, 0)) : S.regex_starts(text, rev, plan);
        if (int rc = finish(c, S)) return rc;
        store_str(c->eng, r, starts);
        return FHS_OK;
    }
    Pos r = S.regex_find(text, rev, plan, halves);
    if (int rc = finish(c, S)) return rc;
    *lo = store(c->eng, r[0]);
    if (hi) *hi = store(c->eng, r[1]);
    return FHS_OK;
}
}  // namespace
int fhs_str_regex_find_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags, fhs_char_t *out) {
    if (!ok_all(c, s, n) || (m && !pat) || !out) return bad(c);
    return regex_find_op(c, "fhs_str_regex_find_clear", s, n, pat, m, flags, nullptr, out, nullptr);
}
int fhs_str_regex_find_clear_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags,
                                  fhs_char_t *lo, fhs_char_t *hi) {
    if (!ok_all(c, s, n) || (m && !pat) || !lo || !hi) return bad(c);
    return regex_find_op(c, "fhs_str_regex_find_clear_wide", s, n, pat, m, flags, nullptr, lo, hi);
}
int fhs_str_regex_starts_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, uint32_t flags, fhs_char_t *out) {
    if (!ok_all(c, s, n) || (m && !pat) || (n && !out)) return bad(c);
    return regex_find_op(c, "fhs_str_regex_starts_clear", s, n, pat, m, flags, out, nullptr, nullptr);
}
int fhs_str_is_empty(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !out) return bad(c);
    Strings S(&c->eng);
    FChar r = S.is_empty(load_str(c->eng, s, n));
    *out = store(c->eng, r);
    return FHS_OK;
}
// ---- positions and counts: one char (the reference's u8) or a (lo, hi) pair, value lo + 256 hi ----
namespace {
struct PatArg {                                              // a pattern as handles, or as clear text
    const fhs_char_t *enc;
    const char *clear;
    size_t m;
};
int store_pos(fhs_ctx *c, Strings &S, Pos &r, fhs_char_t *lo, fhs_char_t *hi) {
    if (int rc = finish(c, S)) return rc;
    *lo = store(c->eng, r[0]);
    if (hi) *hi = store(c->eng, r[1]);
    return FHS_OK;
}
// find / rfind after the argument checks; hi == nullptr: the u8 form
int find_op(fhs_ctx *c, bool reverse, const fhs_char_t *s, size_t n, const PatArg &pat, fhs_char_t *lo, fhs_char_t *hi) {
    const size_t halves = hi ? 2 : 1;
    // The wide forms test the limit before the operands are loaded: loading refreshes noisy operands, which records
    // bootstraps.  The u8 forms load first and leave the test to Strings.  (rfind counts the NUL pushed at mod.rs:737.)
    if (hi && Strings::limit_reached(n + reverse, pat.m, halves)) return c->eng.ctx.fail(FHS_ERR_LIMIT, Strings::LIMIT_MSG);
    Strings S(&c->eng);
    const FStr text = load_str(c->eng, s, n);
    const FStr p = pat.clear ? S.clear(pat.clear, pat.m) : load_str(c->eng, pat.enc, pat.m);
    Pos r = reverse ? S.rfind(text, p, halves) : S.find(text, p, halves);
    return store_pos(c, S, r, lo, hi);
}
// len, or the number of set flags
int count_op(fhs_ctx *c, bool are_flags, const fhs_char_t *s, size_t n, fhs_char_t *lo, fhs_char_t *hi) {
    Strings S(&c->eng);
    const FStr text = load_str(c->eng, s, n);
    Pos r = are_flags ? S.count_flags(text, hi ? 2 : 1) : S.len(text, hi ? 2 : 1);
    return store_pos(c, S, r, lo, hi);
}
}  // namespace

int fhs_str_find(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !ok_all(c, pat, m) || !out) return bad(c);
    return find_op(c, false, s, n, {pat, nullptr, m}, out, nullptr);
}
int fhs_str_find_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, fhs_char_t *out) {
    if (!ok_all(c, s, n) || (m && !pat) || !out) return bad(c);
    return find_op(c, false, s, n, {nullptr, pat, m}, out, nullptr);
}
int fhs_str_rfind(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !ok_all(c, pat, m) || !out) return bad(c);
    return find_op(c, true, s, n, {pat, nullptr, m}, out, nullptr);
}
int fhs_str_len(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !out) return bad(c);
    return count_op(c, false, s, n, out, nullptr);
}
int fhs_str_find_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *lo,
                      fhs_char_t *hi) {                      // mod.rs:1010-1053 with the u8 of :1023-1027, :1044 widened
    if (!ok_all(c, s, n) || !ok_all(c, pat, m) || !lo || !hi) return bad(c);
    return find_op(c, false, s, n, {pat, nullptr, m}, lo, hi);
}
int fhs_str_find_clear_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const char *pat, size_t m, fhs_char_t *lo,
                            fhs_char_t *hi) {                // mod.rs:1075, the same
    if (!ok_all(c, s, n) || (m && !pat) || !lo || !hi) return bad(c);
    return find_op(c, false, s, n, {nullptr, pat, m}, lo, hi);
}
int fhs_str_rfind_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m, fhs_char_t *lo,
                       fhs_char_t *hi) {                     // mod.rs:727-790 with the u8 of :739-744, :753, :783 widened
    if (!ok_all(c, s, n) || !ok_all(c, pat, m) || !lo || !hi) return bad(c);
    return find_op(c, true, s, n, {pat, nullptr, m}, lo, hi);
}
int fhs_str_len_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *lo, fhs_char_t *hi) {   // mod.rs:478-493, no wrap
    if (!ok_all(c, s, n) || !lo || !hi) return bad(c);
    return count_op(c, false, s, n, lo, hi);
}
int fhs_flags_count_wide(fhs_ctx *c, const fhs_char_t *flags, size_t n, fhs_char_t *lo, fhs_char_t *hi) {
    if (!ok_all(c, flags, n) || !lo || !hi) return bad(c);
    return count_op(c, true, flags, n, lo, hi);
}

// ---- encrypted positions as operands: char_at / substr / take / split_at, position a char or a (lo, hi) pair ----
namespace {
// an empty operand or an empty request: clear NULs, and the position is not even loaded (loading may record a refresh)
int store_nuls(fhs_ctx *c, fhs_char_t *out, size_t count) {
    for (size_t i = 0; i < count; i++) {
        FChar z = ch_trivial(&c->eng, 0);
        out[i] = store(c->eng, z);
    }
    return FHS_OK;
}
int char_at_op(fhs_ctx *c, const fhs_char_t *s, size_t n, const PosArg &pos, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !ok_pos(c, pos) || !out) return bad(c);
    if (n == 0) return store_nuls(c, out, 1);
    Strings S(&c->eng);
    const FStr text = load_str(c->eng, s, n);
    FChar r = S.char_at(text, load_pos(c, pos));
    if (int rc = finish(c, S)) return rc;
    *out = store(c->eng, r);
    return FHS_OK;
}
int substr_op(fhs_ctx *c, const fhs_char_t *s, size_t n, const PosArg &pos, size_t count, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !ok_pos(c, pos) || (count && !out)) return bad(c);
    if (n == 0 || count == 0) return store_nuls(c, out, count);
    Strings S(&c->eng);
    const FStr text = load_str(c->eng, s, n);
    FStr r = S.substr(text, load_pos(c, pos), count);
    if (int rc = finish(c, S)) return rc;
    store_str(c->eng, r, out);
    return FHS_OK;
}
int take_op(fhs_ctx *c, const fhs_char_t *s, size_t n, const PosArg &pos, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !ok_pos(c, pos) || (n && !out)) return bad(c);
    if (n == 0) return FHS_OK;
    Strings S(&c->eng);
    const FStr text = load_str(c->eng, s, n);
    FStr r = S.take(text, load_pos(c, pos));
    if (int rc = finish(c, S)) return rc;
    store_str(c->eng, r, out);
    return FHS_OK;
}
int split_at_op(fhs_ctx *c, const fhs_char_t *s, size_t n, const PosArg &pos, fhs_char_t *head, fhs_char_t *tail) {
    if (!ok_all(c, s, n) || !ok_pos(c, pos) || (n && (!head || !tail))) return bad(c);
    if (n == 0) return FHS_OK;
    Strings S(&c->eng);
    const FStr text = load_str(c->eng, s, n);
    FStr h, t;
    S.split_at(text, load_pos(c, pos), &h, &t);
    if (int rc = finish(c, S)) return rc;
    store_str(c->eng, h, head);
    store_str(c->eng, t, tail);
    return FHS_OK;
}
}  // namespace
int fhs_str_char_at(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos, fhs_char_t *out) {
    return char_at_op(c, s, n, {{pos}, 1}, out);
}
int fhs_str_char_at_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos_lo, fhs_char_t pos_hi, fhs_char_t *out) {
    return char_at_op(c, s, n, {{pos_lo, pos_hi}, 2}, out);
}
int fhs_str_substr(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos, size_t count, fhs_char_t *out) {
    return substr_op(c, s, n, {{pos}, 1}, count, out);
}
int fhs_str_substr_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos_lo, fhs_char_t pos_hi, size_t count,
                        fhs_char_t *out) {
    return substr_op(c, s, n, {{pos_lo, pos_hi}, 2}, count, out);
}
int fhs_str_take(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos, fhs_char_t *out) {
    return take_op(c, s, n, {{pos}, 1}, out);
}
int fhs_str_take_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos_lo, fhs_char_t pos_hi, fhs_char_t *out) {
    return take_op(c, s, n, {{pos_lo, pos_hi}, 2}, out);
}
int fhs_str_split_at(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos, fhs_char_t *head, fhs_char_t *tail) {
    return split_at_op(c, s, n, {{pos}, 1}, head, tail);
}
int fhs_str_split_at_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t pos_lo, fhs_char_t pos_hi, fhs_char_t *head,
                          fhs_char_t *tail) {
    return split_at_op(c, s, n, {{pos_lo, pos_hi}, 2}, head, tail);
}

int fhs_str_compare(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, int cmp, fhs_char_t *out) {
    if (!ok_all(c, a, na) || !ok_all(c, b, nb) || !out || cmp < 0 || cmp > 3) return bad(c);
    Strings S(&c->eng);
    FChar r = S.comparison(load_str(c->eng, a, na), load_str(c->eng, b, nb), cmp);
    *out = store(c->eng, r);
    return FHS_OK;
}

int fhs_str_compare_partial(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, int cmp,
                            fhs_char_t *any_diff, fhs_char_t *verdict) {
    if (!ok_all(c, a, na) || !ok_all(c, b, nb) || !any_diff || !verdict || cmp < 0 || cmp > 3 || na != nb) return bad(c);
    Strings S(&c->eng);
    FChar d, v;
    S.f_cmp_partial(load_str(c->eng, a, na), load_str(c->eng, b, nb), cmp, &d, &v);
    *any_diff = store(c->eng, d);
    *verdict = store(c->eng, v);
    return FHS_OK;
}

int fhs_flags_first_decides(fhs_ctx *c, const fhs_char_t *any_diff, const fhs_char_t *verdict, size_t n, int tie,
                            fhs_char_t *out) {
    if (!ok_all(c, any_diff, n) || !ok_all(c, verdict, n) || !out) return bad(c);
    Strings S(&c->eng);
    FChar r = S.flags_first_decides(load_str(c->eng, any_diff, n), load_str(c->eng, verdict, n), tie);
    *out = store(c->eng, r);
    return FHS_OK;
}

#define STR_MAP_OP(NAME, METHOD)                                                  \
    int NAME(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t *out) {        \
        if (!ok_all(c, s, n) || (n && !out)) return bad(c);                       \
        Strings S(&c->eng);                                                       \
        FStr r = S.METHOD(load_str(c->eng, s, n));                                \
        store_str(c->eng, r, out);                                                \
        return FHS_OK;                                                            \
    }
STR_MAP_OP(fhs_str_to_upper, to_upper)
STR_MAP_OP(fhs_str_to_lower, to_lower)
STR_MAP_OP(fhs_str_trim_end, trim_end)
STR_MAP_OP(fhs_str_trim_start, trim_start)
STR_MAP_OP(fhs_str_trim, trim)
STR_MAP_OP(fhs_bubble_zeroes_right, bubble_zeroes_right)

// ---- clear tables and sets ----
namespace {
// the plan first: it reads no operand, so a full registry fails before a noisy operand is refreshed
int class_op(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *set32, fhs_char_t *flags, fhs_char_t *lo, fhs_char_t *hi) {
    const size_t halves = hi ? 2 : 1;
    if (lo && n > ((size_t)1 << (8 * halves))) return c->eng.ctx.fail(FHS_ERR_LIMIT, Strings::LIMIT_MSG);
    Strings S(&c->eng);
    Strings::TablePlan plan;
    if (!S.plan_class(set32, &plan)) return finish(c, S);
    const FStr text = load_str(c->eng, s, n);
    if (!lo) {
        FStr r = S.class_flags(text, plan);
        store_str(c->eng, r, flags);
        return FHS_OK;
    }
    Pos r = S.find_class(text, plan, halves);
    return store_pos(c, S, r, lo, hi);
}
}  // namespace
int fhs_str_map_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *table, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !table || (n && !out)) return bad(c);
    Strings S(&c->eng);
    Strings::TablePlan plan;
    if (!S.plan_map(table, &plan)) return finish(c, S);
    FStr r = S.map_clear(load_str(c->eng, s, n), plan);
    store_str(c->eng, r, out);
    return FHS_OK;
}
int fhs_str_class_flags(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *set32, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !set32 || (n && !out)) return bad(c);
    return class_op(c, s, n, set32, out, nullptr, nullptr);
}
int fhs_str_find_class(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *set32, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !set32 || !out) return bad(c);
    return class_op(c, s, n, set32, nullptr, out, nullptr);
}
int fhs_str_find_class_wide(fhs_ctx *c, const fhs_char_t *s, size_t n, const uint8_t *set32, fhs_char_t *lo, fhs_char_t *hi) {
    if (!ok_all(c, s, n) || !set32 || !lo || !hi) return bad(c);
    return class_op(c, s, n, set32, nullptr, lo, hi);
}

size_t fhs_str_replace_len(size_t n, size_t mf, size_t mt) {
    const size_t d = n + 1;                       // the reference pushes one NUL (mod.rs:841,898)
    if (mf >= mt) return d;                       // handle_longer_from
    if (mf == 0) return (d + (d + 1) * mt) + 1;   // mod.rs:910-914
    return mt * d + d;                            // mod.rs:903-907
}
int fhs_str_replace(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *from, size_t mf,
                    const fhs_char_t *to, size_t mt, fhs_char_t *out, size_t out_cap, size_t *out_len) {
    if (!ok_all(c, s, n) || !ok_all(c, from, mf) || !ok_all(c, to, mt) || !out || !out_len) return bad(c);
    if (out_cap < fhs_str_replace_len(n, mf, mt)) return c->eng.ctx.fail(FHS_ERR_ARG, "output capacity too small");
    Strings S(&c->eng);
    FStr r = S.replace(load_str(c->eng, s, n), load_str(c->eng, from, mf), load_str(c->eng, to, mt));
    store_str(c->eng, r, out);
    *out_len = r.size();
    return FHS_OK;
}
int fhs_str_replacen(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *from, size_t mf,
                     const fhs_char_t *to, size_t mt, fhs_char_t count, fhs_char_t *out, size_t out_cap,
                     size_t *out_len) {
    if (!ok_all(c, s, n) || !ok_all(c, from, mf) || !ok_all(c, to, mt) || !ok(c, count) || !out || !out_len)
        return bad(c);
    if (out_cap < fhs_str_replace_len(n, mf, mt)) return c->eng.ctx.fail(FHS_ERR_ARG, "output capacity too small");
    Strings S(&c->eng);
    FStr r = S.replacen(load_str(c->eng, s, n), load_str(c->eng, from, mf), load_str(c->eng, to, mt),
                        load(c->eng, count));
    store_str(c->eng, r, out);
    *out_len = r.size();
    return FHS_OK;
}
int fhs_str_repeat(fhs_ctx *c, const fhs_char_t *s, size_t n, fhs_char_t count, fhs_char_t *out) {
    if (!ok_all(c, s, n) || !ok(c, count) || (n && !out)) return bad(c);
    Strings S(&c->eng);
    FStr r = S.repeat(load_str(c->eng, s, n), load(c->eng, count));
    store_str(c->eng, r, out);
    return FHS_OK;
}
int fhs_str_repeat_clear(fhs_ctx *c, const fhs_char_t *s, size_t n, size_t count, fhs_char_t *out) {
    if (!ok_all(c, s, n) || (n && count && !out)) return bad(c);
    Strings S(&c->eng);
    FStr r = S.repeat_clear(load_str(c->eng, s, n), count);
    store_str(c->eng, r, out);
    return FHS_OK;
}
int fhs_str_concatenate(fhs_ctx *c, const fhs_char_t *a, size_t na, const fhs_char_t *b, size_t nb, fhs_char_t *out) {
    if (!ok_all(c, a, na) || !ok_all(c, b, nb) || ((na + nb) && !out)) return bad(c);
    Strings S(&c->eng);
    FStr r = S.concatenate(load_str(c->eng, a, na), load_str(c->eng, b, nb));
    store_str(c->eng, r, out);
    return FHS_OK;
}
int fhs_str_strip_prefix(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m,
                         fhs_char_t *out, fhs_char_t *found) {
    if (!ok_all(c, s, n) || !ok_all(c, pat, m) || (n && !out) || !found) return bad(c);
    Strings S(&c->eng);
    FChar f;
    FStr r = S.strip_prefix(load_str(c->eng, s, n), load_str(c->eng, pat, m), &f);
    store_str(c->eng, r, out);
    *found = store(c->eng, f);
    return FHS_OK;
}
int fhs_str_strip_suffix(fhs_ctx *c, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m,
                         fhs_char_t *out, fhs_char_t *found) {
    if (!ok_all(c, s, n) || !ok_all(c, pat, m) || (n && !out) || !found) return bad(c);
    Strings S(&c->eng);
    FChar f;
    FStr r = S.strip_suffix(load_str(c->eng, s, n), load_str(c->eng, pat, m), &f);
    store_str(c->eng, r, out);
    *found = store(c->eng, f);
    return FHS_OK;
}

size_t fhs_str_split_dim(int kind, size_t n) { return kind == Strings::SPLIT_ASCII_WHITESPACE ? n : n + 1; }
int fhs_str_split(fhs_ctx *c, int kind, const fhs_char_t *s, size_t n, const fhs_char_t *pat, size_t m,
                  fhs_char_t count, fhs_char_t *out, size_t out_cap, size_t *dim, fhs_char_t *found) {
    if (!ok_all(c, s, n) || !ok_all(c, pat, m) || !out || !dim || !found || kind < 0 || kind > 8) return bad(c);
    const bool needs_n = kind == Strings::SPLITN || kind == Strings::RSPLITN;
    if (needs_n && !ok(c, count)) return bad(c);
    const size_t d = fhs_str_split_dim(kind, n);
    if (out_cap < d * d) return c->eng.ctx.fail(FHS_ERR_ARG, "output capacity too small");
    Strings S(&c->eng);
    FChar nn, f;
    if (needs_n) nn = load(c->eng, count);
    std::vector<FStr> r = S.split_family(kind, load_str(c->eng, s, n), load_str(c->eng, pat, m),
                                         needs_n ? &nn : nullptr, &f);
    for (size_t i = 0; i < d; i++)
        for (size_t j = 0; j < d; j++) out[i * d + j] = store(c->eng, r[i][j]);
    *dim = d;
    *found = store(c->eng, f);
    return FHS_OK;
}

int fhs_flags_or(fhs_ctx *c, const fhs_char_t *flags, size_t n, fhs_char_t *out) {
    if (!ok_all(c, flags, n) || !out) return bad(c);
    Strings S(&c->eng);
    FChar r = S.flags_or(load_str(c->eng, flags, n));
    *out = store(c->eng, r);
    return FHS_OK;
}
int fhs_flags_and(fhs_ctx *c, const fhs_char_t *flags, size_t n, fhs_char_t *out) {
    if (!ok_all(c, flags, n) || !out) return bad(c);
    Strings S(&c->eng);
    FChar r = S.flags_and(load_str(c->eng, flags, n));
    *out = store(c->eng, r);
    return FHS_OK;
}

int fhs_dist_config(fhs_ctx *c, int rank, int world) {
    if (!c || world < 1 || rank < 0 || rank >= world) return bad(c);
    c->eng.dist_rank = rank;
    c->eng.dist_world = world;
    return FHS_OK;
}
int fhs_flush_plan(fhs_ctx *c, uint64_t *n_levels, uint64_t *max_level_width) {
    if (!c || !n_levels || !max_level_width) return bad(c);
    int rc = c->eng.plan_flush();
    if (rc) return rc;
    *n_levels = c->eng.planned_levels();
    *max_level_width = c->eng.planned_levels() ? c->eng.planned_max_width() : 0;
    return FHS_OK;
}
int fhs_flush_level_exec(fhs_ctx *c, uint64_t level, uint64_t *d_slice, uint64_t *width, uint64_t *cap) {
    if (!c || !d_slice || !width || !cap || level >= c->eng.planned_levels()) return bad(c);
    const size_t w = c->eng.level_width(level), world = (size_t)c->eng.dist_world;
    const size_t cp = (w + world - 1) / world;
    const size_t lo = std::min(w, (size_t)c->eng.dist_rank * cp), hi = std::min(w, lo + cp);
    *width = w;
    *cap = cp;
    return c->eng.exec_level(level, lo, hi, d_slice);
}
int fhs_flush_level_commit(fhs_ctx *c, uint64_t level, const uint64_t *d_all) {
    if (!c || !d_all || level >= c->eng.planned_levels()) return bad(c);
    return c->eng.commit_level(level, d_all);
}
int fhs_stream_sync(fhs_ctx *c) {
    if (!c) return FHS_ERR_ARG;
    if (c->eng.planner) return FHS_OK;
    if (hipStreamSynchronize(c->eng.ctx.stream) != hipSuccess) return c->eng.ctx.fail(FHS_ERR_HIP, "stream sync failed");
    return FHS_OK;
}

int fhs_get_stats(fhs_ctx *c, fhs_stats *out) {
    if (!c || !out) return bad(c);
    out->pbs_executed = c->eng.stats.pbs_executed;
    out->pbs_folded = c->eng.stats.pbs_folded;
    out->levels = c->eng.stats.levels;
    out->max_level_width = c->eng.stats.max_level_width;
    out->blocks_live = c->eng.blocks_live();
    out->max_input_sum_c2 = c->eng.stats.max_input_sum_c2;
    out->pbs_shared = c->eng.stats.pbs_shared;
    out->pbs_extracted = c->eng.stats.pbs_extracted;
    return FHS_OK;
}
int fhs_char_sum_c2(fhs_ctx *c, fhs_char_t h, uint64_t *out) {
    if (!ok(c, h) || !out) return bad(c);
    const Bid *b = c->eng.char_blocks(h);
    int64_t m = 0;
    for (int i = 0; i < 4; i++) m = std::max<int64_t>(m, c->eng.sum_c2(b[i]));
    *out = (uint64_t)m;
    return FHS_OK;
}
int fhs_char_set_noise(fhs_ctx *c, fhs_char_t h, uint64_t sum_c2) {
    if (!ok(c, h)) return bad(c);
    const Bid *b = c->eng.char_blocks(h);
    for (int i = 0; i < 4; i++)                               // all four blocks are checked before any is changed:
        if (int rc = c->eng.set_var(b[i], sum_c2, true)) return rc;   // a refused declaration leaves the handle as it was
    for (int i = 0; i < 4; i++) (void)c->eng.set_var(b[i], sum_c2);
    return FHS_OK;
}
int fhs_trivial_value(fhs_ctx *c, fhs_char_t h, int *is_trivial, uint8_t *value) {
    if (!ok(c, h) || !is_trivial || !value) return bad(c);
    const Bid *b = c->eng.char_blocks(h);
    unsigned v = 0;
    *is_trivial = 1;
    for (int i = 0; i < 4; i++) {
        if (!c->eng.is_triv(b[i])) { *is_trivial = 0; *value = 0; return FHS_OK; }
        v += (unsigned)(c->eng.triv_val(b[i]) & 15) << (2 * i);      // carries add up like in a decryption
    }
    *value = (uint8_t)(v & 255);
    return FHS_OK;
}
int fhs_level_widths(fhs_ctx *c, uint32_t *out, size_t cap, size_t *n) {
    if (!c || !n) return bad(c);
    const auto &w = c->eng.stats.level_widths;
    *n = w.size();
    if (out) std::copy(w.begin(), w.begin() + std::min(cap, w.size()), out);
    return FHS_OK;
}
int fhs_set_rotation_sharing(fhs_ctx *c, int on) {
    if (!c) return FHS_ERR_ARG;
    c->eng.share_rotations = on != 0;
    return FHS_OK;
}
int fhs_launch_groups(fhs_ctx *c, uint32_t *out, size_t cap, size_t *n) {
    if (!c || !n) return bad(c);
    const auto &w = c->eng.stats.group_rows;
    *n = w.size();
    if (out) std::copy(w.begin(), w.begin() + std::min(cap, w.size()), out);
    return FHS_OK;
}
int fhs_reset_stats(fhs_ctx *c) {
    if (!c) return FHS_ERR_ARG;
    c->eng.stats = EngineStats();
    return FHS_OK;
}

}  // extern "C"
