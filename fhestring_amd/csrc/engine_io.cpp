// The engine's traffic with the host and with memory at rest: block and whole-string uploads, downloads, packing,
// the device-resident string store, char handles.  The graph, the planner and the launch groups are engine.cpp.
#include "engine.h"
#include "host_parallel.h"
#include "pack_kernels.h"
#include "../../include/fhestring_hip.h"
#include "pk_kernels.h"
#include "rekey_kernels.h"
#include "seeded_kernels.h"
#include "select_kernels.h"
#include "store_kernels.h"

#include <algorithm>
#include <cstring>

namespace fhs {

// a packed GLWE, a parked entry's GLWE and a public-key GLWE hold the same blocks: the store moves words between them
static_assert(PACK_GROUP == REKEY_GROUP && PACK_GROUP == FHS_PK_GROUP && PACK_GROUP == FHS_PACK_GROUP,
              "one group size for the packing tree, the re-key and the public-key expansion");

bool TransferBuffer::ensure(size_t rows, hipStream_t s) {
    const size_t words = rows * BIG_CT + rows;
    if (words_ < words) {
        if (done_.peek()) (void)hipEventSynchronize(done_.peek());
        pin_.release();
        if (dev_) { (void)hipStreamSynchronize(s); dev_.release(); }
        words_ = 0;
        cursor_ = CURSOR_RESET;
        const size_t want = std::max<size_t>(rows, 260) * (BIG_CT + 1);
        if (pin_.reserve_exact(want * 8) == hipSuccess && dev_.reserve_exact(want * 8) == hipSuccess) words_ = want;
        else { pin_.release(); dev_.release(); }
    }
    return pin_ && done_.get();
}
bool TransferBuffer::begin_pass(size_t rows, hipStream_t s) {
    if (!ensure(std::max<size_t>(rows, 1), s)) return false;
    (void)hipEventSynchronize(done_.peek());         // (no-op before the first copy)
    cursor_ = CURSOR_RESET;
    return true;
}
bool TransferBuffer::begin_table_pass(size_t n, size_t &at, hipStream_t s) {
    if (!ensure(1, s) || n > words_) return false;
    if (cursor_ == CURSOR_RESET || cursor_ + n > words_) {
        (void)hipEventSynchronize(done_.peek());
        cursor_ = 0;
    }
    at = cursor_;
    cursor_ += n;
    return true;
}
hipError_t TransferBuffer::copy_up(size_t at, size_t words, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(dev() + at, pin() + at, words * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) (void)hipEventRecord(done_.peek(), s);
    return e;
}

// one fresh block filled by a copy on the stream (a planner copies nothing)
Bid Engine::copy_in(const uint64_t *src, hipMemcpyKind kind) {
    if (!planner) (void)hipSetDevice(ctx.device);   // one process may see several GPUs (torch sets its own current device)
    uint64_t *d = alloc_block();
    if (!d) return 0;
    if (!planner && hipMemcpyAsync(d, src, BIG_CT * 8, kind, ctx.stream) != hipSuccess) {
        free_block(d);
        return 0;
    }
    Bid id = new_node();
    nodes_[id].kind = BlockNode::MAT;
    nodes_[id].dev = d;
    return id;
}
Bid Engine::from_device(const uint64_t *d_ct) { return copy_in(d_ct, hipMemcpyDeviceToDevice); }
Bid Engine::from_host(const uint64_t *ct) {
    const Bid id = copy_in(ct, hipMemcpyHostToDevice);
    if (id && planner && trace_plan) { trace_.push_back(TR_UPLOAD); trace_.push_back((uint64_t)(uintptr_t)nodes_[id].dev); }
    return id;
}

// ---- whole-string uploads: what the three variants share -----------------------------------------------------------
int Engine::undo_upload(Bid *out, size_t count) {
    for (size_t i = 0; i < count; i++) {
        if (out[i]) release(out[i]);
        out[i] = 0;
    }
    return -1;
}

// `n` fresh pool blocks as MAT nodes in out[0..n); their device pointers go to ptrs[0..n) (the pass's pointer table in
// the pinned buffer).  false: the pool is exhausted (the caller undoes the whole upload).
bool Engine::new_mat_blocks(size_t n, Bid *out, uint64_t *ptrs) {
    for (size_t k = 0; k < n; k++) {
        uint64_t *d = alloc_block();
        if (!d) return false;
        out[k] = new_node();
        nodes_[out[k]].kind = BlockNode::MAT;
        nodes_[out[k]].dev = d;
        ptrs[k] = (uint64_t)(uintptr_t)d;
    }
    return true;
}

// the planner's upload: blocks and nodes only, one TR_UPLOAD per block in block order
int Engine::plan_upload(size_t count, Bid *out) {
    for (size_t i = 0; i < count; i++) {
        uint64_t tok = 0;
        (void)new_mat_blocks(1, out + i, &tok);
        if (trace_plan) { trace_.push_back(TR_UPLOAD); trace_.push_back(tok); }
    }
    return 0;
}

// One pass through the transfer buffer, after its begin_pass / begin_table_pass: the pass's `n` blocks are allocated,
// their pointers written at word `ptr_at` of the pinned side, words [at, at + words) copied to the device mirror and the
// event behind the copy recorded.
bool Engine::send_pass(size_t n, Bid *out, size_t ptr_at, size_t at, size_t words) {
    return new_mat_blocks(n, out, xfer_.pin() + ptr_at) && xfer_.copy_up(at, words, ctx.stream) == hipSuccess;
}

int Engine::from_host_many(const uint64_t *cts, size_t count, Bid *out) {
    for (size_t i = 0; i < count; i++) out[i] = 0;
    auto one_by_one = [&](size_t from) {
        for (size_t i = from; i < count; i++)
            if (!(out[i] = from_host(cts + i * BIG_CT))) return undo_upload(out, count);
        return 0;
    };
    if (planner || count < 4) return one_by_one(0);
    (void)hipSetDevice(ctx.device);
    // staging: [count x 2049 words][count destination pointers], pinned on the host and mirrored on the device: one copy,
    // one scatter launch (pool blocks are not neighbours once the free list has been through a few operations)
    constexpr size_t MAX_BATCH = 2048;               // 33.6 MB per pass
    for (size_t done = 0, n; done < count; done += n) {
        n = std::min(MAX_BATCH, count - done);
        if (!xfer_.begin_pass(n, ctx.stream)) return one_by_one(done);                 // no staging memory: block by block
        {
            // pageable -> pinned: one thread copies ~10 GB/s, which for the 537 MB of two 4097-character strings is as long
            // as their (threaded) client encryption; large passes are split over a few host threads
            const size_t bytes = n * BIG_CT * 8;
            const size_t nt = bytes >= ((size_t)8 << 20) ? host_threads(8) : 1;
            const char *src = reinterpret_cast<const char *>(cts + done * BIG_CT);
            char *dst = reinterpret_cast<char *>(xfer_.pin());
            const size_t part = (bytes / nt + 4095) & ~(size_t)4095;
            parallel_for(nt, nt, 1, [&](size_t t) {
                const size_t lo = std::min(bytes, t * part), hi = std::min(bytes, (t + 1) * part);
                std::memcpy(dst + lo, src + lo, hi - lo);
            });
        }
        uint64_t *const dev = xfer_.dev();
        if (!send_pass(n, out + done, n * BIG_CT, 0, n * BIG_CT + n) ||
            launch_scatter_blocks(dev, reinterpret_cast<uint64_t *const *>(dev + n * BIG_CT), (int)n, ctx.stream) != hipSuccess)
            return undo_upload(out, count);
    }
    return 0;
}

int Engine::from_compressed_many(const uint32_t seed[8], const uint64_t *bodies, size_t count, uint64_t first_block,
                                 Bid *out) {
    for (size_t i = 0; i < count; i++) out[i] = 0;
    if (planner) return plan_upload(count, out);
    (void)hipSetDevice(ctx.device);
    SeedKey key;
    for (int i = 0; i < 8; i++) key.w[i] = seed[i];
    // staging: [n bodies][n destination pointers] (16 B per block) in the pinned buffer of from_host_many: 4096 blocks
    // per pass
    constexpr size_t MAX_BATCH = 4096;
    for (size_t done = 0, n; done < count; done += n) {
        n = std::min(MAX_BATCH, count - done);
        if (!xfer_.begin_pass(0, ctx.stream)) return undo_upload(out, count);
        std::memcpy(xfer_.pin(), bodies + done, n * 8);
        if (!send_pass(n, out + done, n, 0, 2 * n) ||
            launch_expand_seeded_blocks(key, first_block + done, xfer_.dev(), (int)n, ctx.stream) != hipSuccess)
            return undo_upload(out, count);
    }
    return 0;
}

int Engine::from_public_many(const uint32_t *mask32, const uint32_t *body32, size_t count, uint64_t first_block, Bid *out) {
    for (size_t i = 0; i < count; i++) out[i] = 0;
    if (planner) return plan_upload(count, out);
    (void)hipSetDevice(ctx.device);
    // staging, in the pinned buffer of from_host_many: [n destination pointers][n u32 bodies][u32 masks of the groups
    // the pass touches, 2048 each] -- at most three groups for 4096 blocks
    constexpr size_t MAX_BATCH = 4096;
    for (size_t done = 0, n; done < count; done += n) {
        n = std::min(MAX_BATCH, count - done);
        const uint64_t t0 = first_block + done;
        const size_t g0 = (size_t)(t0 / FHS_PK_GROUP), groups = (size_t)((t0 + n - 1) / FHS_PK_GROUP) - g0 + 1;
        const size_t body_at = n, mask_at = n + (n + 1) / 2, words = mask_at + groups * (BIG_N / 2);
        if (!xfer_.begin_pass(0, ctx.stream)) return undo_upload(out, count);
        std::memcpy(xfer_.pin() + body_at, body32 + t0, n * 4);
        std::memcpy(xfer_.pin() + mask_at, mask32 + g0 * BIG_N, groups * BIG_N * 4);
        uint64_t *const dev = xfer_.dev();
        if (!send_pass(n, out + done, 0, 0, words) ||
            launch_expand_public_blocks(reinterpret_cast<const uint32_t *>(dev + mask_at),
                                        reinterpret_cast<const uint32_t *>(dev + body_at),
                                        reinterpret_cast<uint64_t *const *>(dev), (uint32_t)(t0 % FHS_PK_GROUP), (int)n,
                                        ctx.stream) != hipSuccess)
            return undo_upload(out, count);
    }
    return 0;
}

int Engine::materialize_lin(Bid b) {
    BlockNode &n = nodes_[b];
    if (n.kind != BlockNode::LIN) return 0;
    if (planner) return ctx.fail(-3, "planner context: nothing is computed");
    std::vector<LinTerm> terms;
    for (const Term &t : n.terms) {
        const BlockNode &tb = nodes_[t.blk];
        if (tb.kind != BlockNode::MAT) return ctx.fail(-3, "internal: lincomb term pending after flush");
        terms.push_back({tb.dev, t.coef});
    }
    LinDesc d{0, (uint32_t)terms.size(), (uint64_t)(n.konst & 31) << DELTA_LOG};
    const size_t total = sizeof(LinDesc) + terms.size() * sizeof(LinTerm);
    std::vector<uint8_t> host(total);
    std::memcpy(host.data(), &d, sizeof(d));
    std::memcpy(host.data() + sizeof(d), terms.data(), terms.size() * sizeof(LinTerm));
    hipError_t e = hipStreamSynchronize(ctx.stream);   // plan_buf_ may be in use by queued launches
    if (e == hipSuccess) e = plan_buf_.reserve(total);
    if (e == hipSuccess) e = hipMemcpyAsync(plan_buf_.ptr, host.data(), total, hipMemcpyHostToDevice, ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "materialize upload");
    uint64_t *o = alloc_block();
    if (!o) return ctx.fail(-2, "device block pool exhausted");
    e = launch_lincomb(plan_buf_.as<LinDesc>(),
                       reinterpret_cast<const LinTerm *>(plan_buf_.as<uint8_t>() + sizeof(LinDesc)), o, 1,
                       ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "lincomb launch");
    // the materialised block IS the linear combination: it keeps its noise (a download followed by further use of the
    // same handle must not look like a fresh bootstrap output to the bookkeeping)
    const int64_t v = sum_c2(b);
    uint8_t packs = 0;                                // the largest packing count among the terms (string store)
    for (const Term &t : n.terms) packs = std::max(packs, nodes_[t.blk].packs);
    std::vector<Term> old;
    old.swap(n.terms);
    n.kind = BlockNode::MAT;
    n.var = (uint16_t)std::min<int64_t>(std::max<int64_t>(v, 1), 65535);
    n.dev = o;
    n.level = 0;
    n.packs = packs;
    for (const Term &t : old) release(t.blk);
    return 0;
}

int Engine::read_block(Bid b, uint64_t *host_out) {
    if (planner) return ctx.fail(-3, "planner context: nothing is computed, there is nothing to download");
    (void)hipSetDevice(ctx.device);
    int rc = flush();
    if (rc) return rc;
    if (nodes_[b].kind == BlockNode::TRIV) {
        std::memset(host_out, 0, BIG_CT * 8);
        host_out[BIG_N] = (uint64_t)nodes_[b].triv << DELTA_LOG;
        return 0;
    }
    if (nodes_[b].kind == BlockNode::LIN && (rc = materialize_lin(b))) return rc;
    if (nodes_[b].kind != BlockNode::MAT) return ctx.fail(-3, "internal: block not materialised");
    hipError_t e = hipMemcpyAsync(host_out, nodes_[b].dev, BIG_CT * 8, hipMemcpyDeviceToHost, ctx.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "download");
    return 0;
}

int Engine::read_many(const Bid *b, size_t count, uint64_t *host_out) {
    if (planner) return ctx.fail(-3, "planner context: nothing is computed, there is nothing to download");
    if (count == 0) return 0;
    (void)hipSetDevice(ctx.device);
    if (int rc = flush()) return rc;
    for (size_t i = 0; i < count; i++)                               // linear combinations become blocks of their own first
        if (nodes_[b[i]].kind == BlockNode::LIN)
            if (int rc = materialize_lin(b[i])) return rc;
    constexpr size_t MAX_BATCH = 2048;
    for (size_t done = 0; done < count;) {
        const size_t n = std::min(MAX_BATCH, count - done);
        if (count < 4 || !xfer_.begin_pass(n, ctx.stream)) {               // (the buffer is shared with the uploads)
            // too few blocks to matter, or no staging memory: block by block
            for (size_t i = done; i < done + n; i++)
                if (int rc = read_block(b[i], host_out + i * BIG_CT)) return rc;
            done += n;
            continue;
        }
        uint64_t *const pin = xfer_.pin(), *const dev = xfer_.dev(), *const tab = pin + n * BIG_CT;
        size_t n_dev = 0;
        for (size_t k = 0; k < n; k++) {
            const BlockNode &nd = nodes_[b[done + k]];
            if (nd.kind == BlockNode::TRIV) { tab[k] = 0; continue; }
            if (nd.kind != BlockNode::MAT) return ctx.fail(-3, "internal: block not materialised");
            tab[k] = (uint64_t)(uintptr_t)nd.dev;
            n_dev++;
        }
        // trivial blocks have no device row: point them at the first real block (their rows are overwritten on the host)
        uint64_t any = 0;
        for (size_t k = 0; k < n && !any; k++) any = tab[k];
        if (n_dev) {
            for (size_t k = 0; k < n; k++)
                if (!tab[k]) tab[k] = any;
            // (the download ends with a stream wait: no event behind this copy)
            hipError_t e = hipMemcpyAsync(dev + n * BIG_CT, tab, n * 8, hipMemcpyHostToDevice, ctx.stream);
            if (e == hipSuccess)
                e = launch_gather_rows(reinterpret_cast<const uint64_t *const *>(dev + n * BIG_CT), dev, (int)n, ctx.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(pin, dev, n * BIG_CT * 8, hipMemcpyDeviceToHost, ctx.stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx.stream);
            if (e != hipSuccess) return ctx.hip_fail(e, "download");
            std::memcpy(host_out + done * BIG_CT, pin, n * BIG_CT * 8);
        }
        for (size_t k = 0; k < n; k++) {
            const BlockNode &nd = nodes_[b[done + k]];
            if (nd.kind != BlockNode::TRIV) continue;
            uint64_t *row = host_out + (done + k) * BIG_CT;
            std::memset(row, 0, BIG_CT * 8);
            row[BIG_N] = (uint64_t)nd.triv << DELTA_LOG;
        }
        done += n;
    }
    return 0;
}

// ---- packing: what the packed download and the string store share --------------------------------------------------
int Engine::prepare_packing(const Bid *b, size_t count) {
    (void)hipSetDevice(ctx.device);
    if (int rc = flush()) return rc;
    for (size_t i = 0; i < count; i++)                               // as read_many: linear combinations become blocks first
        if (nodes_[b[i]].kind == BlockNode::LIN)
            if (int rc = materialize_lin(b[i])) return rc;
    for (size_t i = 0; i < count; i++)
        if (nodes_[b[i]].kind != BlockNode::TRIV && nodes_[b[i]].kind != BlockNode::MAT)
            return ctx.fail(-3, "internal: block not materialised");
    return 0;
}

// One pass: the leaf table of n blocks (groups = ceil(n / 2048) <= 4) and the 11 tree levels, enqueued on the stream;
// the level-11 GLWEs [groups][2][2048] are left in ctx.pack_ws[0].
// Level lv of a group writes (2048 >> lv) GLWEs of 32 KB: level 1 is 32 MB, level 2 16 MB, ping-pong between two
// buffers; four groups in flight keep the workspace at 192 MB.
hipError_t Engine::pack_tree_pass(const Bid *b, size_t n, size_t groups) {
    constexpr size_t GLWE_BYTES = 2 * POLY_N * 8;
    std::vector<PackLeaf> leaves(n);
    for (size_t k = 0; k < n; k++) {
        const BlockNode &nd = nodes_[b[k]];
        if (nd.kind == BlockNode::TRIV) leaves[k] = {nullptr, (uint64_t)nd.triv << DELTA_LOG};
        else leaves[k] = {nd.dev, 0};
    }
    hipError_t e = ctx.pack_tab.reserve(n * sizeof(PackLeaf));
    if (e == hipSuccess) e = ctx.pack_ws[0].reserve(groups * (POLY_N / 2) * GLWE_BYTES);
    if (e == hipSuccess) e = ctx.pack_ws[1].reserve(groups * (POLY_N / 4) * GLWE_BYTES);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ctx.pack_tab.ptr, leaves.data(), n * sizeof(PackLeaf), hipMemcpyHostToDevice, ctx.stream);
    for (int lv = 1; lv <= PACK_TREE_LEVELS && e == hipSuccess; lv++) {
        PackLevelParams p{};
        p.lv = lv; p.groups = (int)groups; p.total = (uint32_t)n;
        p.leaves = ctx.pack_tab.as<PackLeaf>();
        p.src = ctx.pack_ws[lv & 1].as<uint64_t>();
        p.dst = ctx.pack_ws[(lv - 1) & 1].as<uint64_t>();
        p.key_ntt = ctx.d_pack_key_ntt.as<double>(); p.tw = ctx.tw;
        e = launch_pack_level(p, ctx.stream);
    }
    return e;
}

int Engine::read_packed(const Bid *b, size_t count, uint16_t *mask16, uint16_t *body16, uint64_t *mask64, uint64_t *body64,
                        bool recipient) {
    if (planner) return ctx.fail(-3, "planner context: nothing is computed, there is nothing to download");
    if (!ctx.d_pack_key_ntt) return ctx.fail(-3, "packing key not loaded (fhs_load_packing_key)");
    if (recipient && !ctx.d_rekey_key_ntt) return ctx.fail(-3, "re-key key not loaded (fhs_load_rekey_key)");
    if (count == 0) return 0;
    if (int rc = prepare_packing(b, count)) return rc;
    constexpr size_t MAX_GROUPS = 4, GLWE_BYTES = 2 * POLY_N * 8;
    std::vector<uint64_t> wide;
    for (size_t done = 0; done < count;) {
        const size_t n = std::min(MAX_GROUPS * PACK_GROUP, count - done);
        const size_t groups = (n + PACK_GROUP - 1) / PACK_GROUP;
        hipError_t e = ctx.pack_out.reserve(groups * 2 * PACK_GROUP * sizeof(uint16_t));
        if (e == hipSuccess) e = pack_tree_pass(b + done, n, groups);
        uint16_t *d_mask = ctx.pack_out.as<uint16_t>(), *d_body = d_mask + groups * PACK_GROUP;
        if (e == hipSuccess && !recipient)
            e = launch_pack_switch16(ctx.pack_ws[0].as<uint64_t>(), d_mask, d_body, (int)groups, (uint32_t)n, ctx.stream);
        if (e == hipSuccess && recipient) e = rekey_packed_words(ctx.pack_ws[0].as<uint64_t>(), d_mask, d_body, n);
        if (e == hipSuccess)
            e = hipMemcpyAsync(mask16 + done, d_mask, groups * PACK_GROUP * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(body16 + done, d_body, n * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx.stream);
        if (e == hipSuccess && mask64 && body64) {
            wide.resize(groups * 2 * POLY_N);
            e = hipMemcpyAsync(wide.data(), ctx.pack_ws[0].ptr, groups * GLWE_BYTES, hipMemcpyDeviceToHost, ctx.stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx.stream);
        if (e != hipSuccess) return ctx.hip_fail(e, "packed download");
        if (mask64 && body64)
            for (size_t g = 0; g < groups; g++) {
                std::memcpy(mask64 + done + g * POLY_N, wide.data() + g * 2 * POLY_N, POLY_N * 8);
                std::memcpy(body64 + done + g * POLY_N, wide.data() + (g * 2 + 1) * POLY_N, POLY_N * 8);
            }
        done += n;
    }
    return 0;
}

// ---- device-resident string store -------------------------------------------------------------------------------------
const Engine::StoreEntry *Engine::store_entry(uint64_t id) const {
    auto it = store_.find(id);
    return it == store_.end() ? nullptr : &it->second;
}

void Engine::store_stats(size_t *entries, size_t *blocks, size_t *bytes) const {
    size_t nb = 0, by = 0;
    for (const auto &kv : store_) { nb += kv.second.n_blocks; by += kv.second.bytes(); }
    if (entries) *entries = store_.size();
    if (blocks) *blocks = nb;
    if (bytes) *bytes = by;
}

int Engine::store_drop(uint64_t id) {
    auto it = store_.find(id);
    if (it == store_.end()) return ctx.fail(-1, "string store: unknown entry id");
    if (it->second.buf) {                                            // a queued expansion may still read it
        (void)hipSetDevice(ctx.device);
        (void)hipStreamSynchronize(ctx.stream);
    }
    store_.erase(it);
    return 0;
}

int Engine::store_put(const Bid *b, size_t count, uint64_t *id_out) {
    if (!planner && !ctx.d_pack_key_ntt) return ctx.fail(-3, "packing key not loaded (fhs_load_packing_key)");
    if (count == 0) return ctx.fail(-1, "string store: an entry holds at least one character");
    if (planner) {
        if (int rc = flush()) return rc;                             // sums stay sums on a planner: their figure is what counts
    } else if (int rc = prepare_packing(b, count)) return rc;
    // what the bookkeeping knows about every block (a sum that was just materialised carries its figure and the largest
    // packing count of its terms; the planner's unmaterialised sum is read the same way)
    StoreEntry ent;
    ent.n_blocks = count;
    ent.var.resize(count); ent.cycles.resize(count); ent.rot.resize(count);
    for (size_t i = 0; i < count; i++) {
        const BlockNode &nd = nodes_[b[i]];
        int packs = 0;
        if (nd.kind == BlockNode::MAT) packs = nd.packs;
        else if (nd.kind == BlockNode::LIN)
            for (const Term &t : nd.terms) packs = std::max<int>(packs, nodes_[t.blk].packs);
        else if (nd.kind != BlockNode::TRIV) return ctx.fail(-3, "internal: block not materialised");
        if (packs + 1 > STORE_MAX_CYCLES)
            return ctx.fail(-4, "string store: a block would exceed FHS_STORE_MAX_CYCLES packings without a bootstrap in between");
        // a trivial block is packed as the trivial leaf it is and comes back as an ordinary ciphertext
        ent.var[i] = nd.kind == BlockNode::TRIV ? 1 : (uint16_t)std::min<int64_t>(std::max<int64_t>(sum_c2(b[i]), 1), 65535);
        ent.cycles[i] = (uint8_t)(packs + 1);
        ent.rot[i] = nd.kind == BlockNode::MAT ? nd.rot : 0;
    }
    if (!planner) {
        hipError_t e = ent.buf.reserve_exact(ent.bytes());
        uint32_t *mask32 = ent.buf.as<uint32_t>(), *body32 = mask32 + ent.groups() * POLY_N;
        constexpr size_t MAX_GROUPS = 4;
        for (size_t done = 0; done < count && e == hipSuccess;) {     // pass p starts at group 4 p of the entry
            const size_t n = std::min(MAX_GROUPS * PACK_GROUP, count - done);
            const size_t groups = (n + PACK_GROUP - 1) / PACK_GROUP;
            e = pack_tree_pass(b + done, n, groups);
            if (e == hipSuccess)
                e = launch_store_switch32(ctx.pack_ws[0].as<uint64_t>(), mask32, body32, (uint32_t)(done / PACK_GROUP), (int)groups,
                                          (uint32_t)n, ctx.stream);
            done += n;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx.stream);
        if (e != hipSuccess) return ctx.hip_fail(e, "string store: put");
    }
    const uint64_t id = ++store_ids_;
    store_.emplace(id, std::move(ent));
    *id_out = id;
    return 0;
}

int Engine::store_get(uint64_t id, size_t first, size_t count, Bid *out) {
    const StoreEntry *ent = store_entry(id);
    if (!ent) return ctx.fail(-1, "string store: unknown entry id");
    if (first > ent->n_blocks || count > ent->n_blocks - first) return ctx.fail(-1, "string store: window outside the entry");
    for (size_t i = 0; i < count; i++) out[i] = 0;
    if (planner) {
        (void)plan_upload(count, out);
    } else {
        (void)hipSetDevice(ctx.device);
        const uint32_t *mask32 = ent->buf.as<uint32_t>(), *body32 = mask32 + ent->groups() * POLY_N;
        // as from_public_many, but masks and bodies are already on the device: the pinned buffer carries the destination
        // pointers alone (8 B per block)
        constexpr size_t MAX_BATCH = 4096;
        for (size_t done = 0, n; done < count; done += n) {
            n = std::min(MAX_BATCH, count - done);
            const size_t t0 = first + done, g0 = t0 / FHS_PK_GROUP;
            size_t at = 0;
            if (!xfer_.begin_table_pass(n, at, ctx.stream) || !send_pass(n, out + done, at, at, n) ||
                launch_expand_public_blocks(mask32 + g0 * POLY_N, body32 + t0,
                                            reinterpret_cast<uint64_t *const *>(xfer_.dev() + at), (uint32_t)(t0 % FHS_PK_GROUP),
                                            (int)n, ctx.stream) != hipSuccess) {
                (void)undo_upload(out, count);
                return ctx.fail(-2, "string store: get failed (device allocation, copy or expansion launch)");
            }
        }
    }
    for (size_t i = 0; i < count; i++) {
        BlockNode &nd = nodes_[out[i]];
        nd.var = ent->var[first + i];
        nd.rot = ent->rot[first + i];
        nd.packs = ent->cycles[first + i];
    }
    return 0;
}

int Engine::store_export(uint64_t id, uint32_t *mask32, uint32_t *body32, uint64_t *meta) {
    const StoreEntry *ent = store_entry(id);
    if (!ent) return ctx.fail(-1, "string store: unknown entry id");
    if (planner) return ctx.fail(-3, "planner context: nothing is computed, there is nothing to export");
    (void)hipSetDevice(ctx.device);
    const size_t mask_bytes = ent->groups() * POLY_N * 4;
    hipError_t e = hipMemcpyAsync(mask32, ent->buf.ptr, mask_bytes, hipMemcpyDeviceToHost, ctx.stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(body32, ent->buf.as<uint8_t>() + mask_bytes, ent->n_blocks * 4, hipMemcpyDeviceToHost, ctx.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "string store: export");
    std::unordered_map<uint32_t, uint32_t> local;                    // engine id -> 1..k in order of first appearance
    for (size_t i = 0; i < ent->n_blocks; i++) {
        uint64_t g = 0;
        if (ent->rot[i]) {
            auto it = local.find(ent->rot[i]);
            g = it != local.end() ? it->second : (local[ent->rot[i]] = (uint32_t)local.size() + 1);
        }
        meta[i] = (uint64_t)ent->var[i] | (uint64_t)ent->cycles[i] << 16 | g << 32;
    }
    return 0;
}

int Engine::store_import(const uint32_t *mask32, const uint32_t *body32, const uint64_t *meta, size_t n_blocks, uint64_t *id_out) {
    if (n_blocks == 0) return ctx.fail(-1, "string store: an entry holds at least one character");
    StoreEntry ent;
    ent.n_blocks = n_blocks;
    ent.var.assign(n_blocks, 1); ent.cycles.assign(n_blocks, 0); ent.rot.assign(n_blocks, 0);
    uint32_t k = 0;
    if (meta) {
        for (size_t i = 0; i < n_blocks; i++) {
            const uint64_t var = meta[i] & 0xffff, cyc = (meta[i] >> 16) & 0xff, grp = meta[i] >> 32;
            if (var < 1 || cyc > (uint64_t)STORE_MAX_CYCLES || (meta[i] >> 24 & 0xff) || grp > n_blocks)
                return ctx.fail(-1, "string store: import refuses a meta word (var >= 1, cycles <= FHS_STORE_MAX_CYCLES, groups 1..k)");
            ent.var[i] = (uint16_t)var; ent.cycles[i] = (uint8_t)cyc; ent.rot[i] = (uint32_t)grp;
            k = std::max(k, (uint32_t)grp);
        }
    }
    if (!planner) {
        (void)hipSetDevice(ctx.device);
        const size_t mask_bytes = ent.groups() * POLY_N * 4;
        // mask32 and body32 are separate host arrays: each goes to its place in the ONE allocation
        hipError_t e = ent.buf.reserve_exact(ent.bytes());
        if (e == hipSuccess) e = hipMemcpyAsync(ent.buf.ptr, mask32, mask_bytes, hipMemcpyHostToDevice, ctx.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ent.buf.as<uint8_t>() + mask_bytes, body32, n_blocks * 4, hipMemcpyHostToDevice, ctx.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx.stream);
        if (e != hipSuccess) return ctx.hip_fail(e, "string store: import");
    }
    // the entry's k groups get k fresh engine ids, drawn once per entry
    std::vector<uint32_t> fresh(k + 1, 0);
    for (uint32_t g = 1; g <= k; g++) fresh[g] = ++rot_counter_ ? rot_counter_ : ++rot_counter_;
    for (size_t i = 0; i < n_blocks; i++) ent.rot[i] = fresh[ent.rot[i]];
    const uint64_t id = ++store_ids_;
    store_.emplace(id, std::move(ent));
    *id_out = id;
    return 0;
}

// Re-key with the context's key: one launch over all groups on the context's stream, behind every queued expansion of
// the entry.  In place the kernel reads and writes the entry's own allocation (rekey_kernels.hip says why that is safe);
// a copy goes to a new entry of the same size and the original stays as it is.
int Engine::store_rekey(uint64_t id, uint64_t *id_out) {
    auto it = store_.find(id);
    if (it == store_.end()) return ctx.fail(-1, "string store: unknown entry id");
    StoreEntry &src = it->second;
    if (!planner && !ctx.d_rekey_key_ntt) return ctx.fail(-3, "re-key key not loaded (fhs_load_rekey_key)");
    if (src.rekeys >= STORE_MAX_REKEYS)
        return ctx.fail(-4, "string store: the entry has been re-keyed FHS_STORE_MAX_REKEYS times");
    StoreEntry copy;
    if (id_out) {
        copy.n_blocks = src.n_blocks;
        copy.var = src.var; copy.cycles = src.cycles; copy.rot = src.rot;
        copy.rekeys = src.rekeys;
    }
    StoreEntry &dst = id_out ? copy : src;
    if (!planner) {
        (void)hipSetDevice(ctx.device);
        hipError_t e = id_out ? dst.buf.reserve_exact(dst.bytes()) : hipSuccess;
        if (e == hipSuccess)
            e = rekey_words(src.buf.as<uint32_t>(), src.buf.as<uint32_t>() + src.groups() * POLY_N, dst.buf.as<uint32_t>(),
                            dst.buf.as<uint32_t>() + dst.groups() * POLY_N, src.n_blocks);
        if (e != hipSuccess) return ctx.hip_fail(e, "string store: re-key");
    }
    dst.rekeys++;
    if (id_out) {
        const uint64_t nid = ++store_ids_;
        store_.emplace(nid, std::move(copy));
        *id_out = nid;
    }
    return 0;
}

int Engine::store_read_packed(uint64_t id, size_t first_char, size_t count, bool recipient, uint16_t *mask16, uint16_t *body16) {
    const StoreEntry *ent = store_entry(id);
    if (!ent) return ctx.fail(-1, "string store: unknown entry id");
    const size_t n_chars = ent->n_blocks / 4;
    if (first_char > n_chars || count > n_chars - first_char) return ctx.fail(-1, "string store: window outside the entry");
    if (count == 0) return 0;
    if (planner) return ctx.fail(-3, "planner context: nothing is computed, there is nothing to download");
    if (recipient && !ctx.d_rekey_key_ntt) return ctx.fail(-3, "re-key key not loaded (fhs_load_rekey_key)");
    (void)hipSetDevice(ctx.device);
    const size_t t0 = 4 * first_char, body_words = 4 * count, g0 = t0 / PACK_GROUP, first_coef = t0 % PACK_GROUP;
    const size_t groups = (first_coef + body_words + PACK_GROUP - 1) / PACK_GROUP, mask_words = groups * POLY_N;
    const uint32_t *mask32 = ent->buf.as<uint32_t>(), *body32 = mask32 + ent->groups() * POLY_N;
    hipError_t e = ctx.pack_out.reserve((mask_words + body_words) * sizeof(uint16_t));
    uint16_t *d_mask = ctx.pack_out.as<uint16_t>(), *d_body = d_mask + mask_words;
    if (e == hipSuccess && !recipient)
        e = launch_store_switch16(mask32 + g0 * POLY_N, body32 + t0, d_mask, d_body, (int)groups, body_words, ctx.stream);
    if (e == hipSuccess && recipient) {
        RekeyEntryPackedParams p{};
        p.src_mask = mask32 + g0 * POLY_N; p.src_body = body32 + g0 * PACK_GROUP; p.dst_mask = d_mask; p.dst_body = d_body;
        p.first_coef = (uint32_t)first_coef; p.body_words = (uint32_t)body_words; p.groups = (int)groups;
        p.key_ntt = ctx.d_rekey_key_ntt.as<double>(); p.tw = ctx.tw;
        e = launch_rekey_entry_packed(p, ctx.stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(mask16, d_mask, mask_words * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(body16, d_body, body_words * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "string store: packed download");
    return 0;
}

hipError_t Engine::rekey_words(const uint32_t *d_mask, const uint32_t *d_body, uint32_t *d_mask_out, uint32_t *d_body_out,
                               size_t n_blocks) {
    RekeyParams p{};
    p.src_mask = d_mask; p.src_body = d_body; p.dst_mask = d_mask_out; p.dst_body = d_body_out;
    p.total = (uint32_t)n_blocks; p.groups = (int)((n_blocks + REKEY_GROUP - 1) / REKEY_GROUP);
    p.key_ntt = ctx.d_rekey_key_ntt.as<double>(); p.tw = ctx.tw;
    return launch_rekey_glwe(p, ctx.stream);
}

// The recipient download's kernel over `n_blocks` blocks of level-11 GLWEs [groups][mask, body][2048]: one launch.
hipError_t Engine::rekey_packed_words(const uint64_t *d_glwe, uint16_t *d_mask16, uint16_t *d_body16, size_t n_blocks) {
    RekeyPackedParams p{};
    p.src = d_glwe; p.dst_mask = d_mask16; p.dst_body = d_body16;
    p.total = (uint32_t)n_blocks; p.groups = (int)((n_blocks + REKEY_GROUP - 1) / REKEY_GROUP);
    p.key_ntt = ctx.d_rekey_key_ntt.as<double>(); p.tw = ctx.tw;
    return launch_rekey_packed(p, ctx.stream);
}

// Diagnostic: that kernel on raw host words of any block count.  The host arrays are [groups][2048] each; the device
// layout interleaves them per group, as the packing tree leaves them.
int Engine::debug_rekey_packed(const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, uint16_t *mask16, uint16_t *body16) {
    if (planner) return ctx.fail(-3, "planner context: nothing is computed");
    if (!ctx.d_rekey_key_ntt) return ctx.fail(-3, "re-key key not loaded (fhs_load_rekey_key)");
    if (n_blocks == 0) return 0;
    (void)hipSetDevice(ctx.device);
    const size_t groups = (n_blocks + REKEY_GROUP - 1) / REKEY_GROUP, words = groups * POLY_N;
    std::vector<uint64_t> glwe(2 * words);
    for (size_t g = 0; g < groups; g++) {
        std::memcpy(glwe.data() + g * 2 * POLY_N, mask64 + g * POLY_N, POLY_N * 8);
        std::memcpy(glwe.data() + (g * 2 + 1) * POLY_N, body64 + g * POLY_N, POLY_N * 8);
    }
    DevBuf buf;
    hipError_t e = buf.reserve_exact(2 * words * 8 + (words + n_blocks) * 2);
    uint64_t *d_glwe = buf.as<uint64_t>();
    uint16_t *d_mask = reinterpret_cast<uint16_t *>(d_glwe + 2 * words), *d_body = d_mask + words;
    if (e == hipSuccess) e = hipMemcpyAsync(d_glwe, glwe.data(), 2 * words * 8, hipMemcpyHostToDevice, ctx.stream);
    if (e == hipSuccess) e = rekey_packed_words(d_glwe, d_mask, d_body, n_blocks);
    if (e == hipSuccess) e = hipMemcpyAsync(mask16, d_mask, words * 2, hipMemcpyDeviceToHost, ctx.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(body16, d_body, n_blocks * 2, hipMemcpyDeviceToHost, ctx.stream);
    hipError_t es = hipStreamSynchronize(ctx.stream);            // before buf and glwe go, on every path
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return ctx.hip_fail(e, "recipient re-key (diagnostic)");
    return 0;
}

// Diagnostic: the kernel on raw host words of any block count, through a scratch allocation of the entry layout.
int Engine::debug_rekey(const uint32_t *mask32, const uint32_t *body32, size_t n_blocks, uint32_t *mask_out, uint32_t *body_out) {
    if (planner) return ctx.fail(-3, "planner context: nothing is computed");
    if (!ctx.d_rekey_key_ntt) return ctx.fail(-3, "re-key key not loaded (fhs_load_rekey_key)");
    if (n_blocks == 0) return 0;
    (void)hipSetDevice(ctx.device);
    const size_t mask_words = (n_blocks + REKEY_GROUP - 1) / REKEY_GROUP * POLY_N;
    DevBuf buf;
    hipError_t e = buf.reserve_exact((mask_words + n_blocks) * 4);
    uint32_t *d_mask = buf.as<uint32_t>(), *d_body = d_mask + mask_words;
    if (e == hipSuccess) e = hipMemcpyAsync(d_mask, mask32, mask_words * 4, hipMemcpyHostToDevice, ctx.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_body, body32, n_blocks * 4, hipMemcpyHostToDevice, ctx.stream);
    if (e == hipSuccess) e = rekey_words(d_mask, d_body, d_mask, d_body, n_blocks);
    if (e == hipSuccess) e = hipMemcpyAsync(mask_out, d_mask, mask_words * 4, hipMemcpyDeviceToHost, ctx.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(body_out, d_body, n_blocks * 4, hipMemcpyDeviceToHost, ctx.stream);
    hipError_t es = hipStreamSynchronize(ctx.stream);            // before buf goes, on every path
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return ctx.hip_fail(e, "re-key (diagnostic)");
    return 0;
}

// ---- string store: select by encrypted index ---------------------------------------------------------------------------
// The queries of a call cross the bus as they are -- full words, or seeds and bodies -- in one table pass of the pinned
// staging buffer, the pointer table of the destinations behind them; select_query_to_ntt_kernel reads the mirror and
// writes ctx.sel_query (stream order keeps the mirror until then: every later pass copies on the same stream).
hipError_t Engine::select_queries_to_ntt(const SelectQueries &q, int bits, uint32_t *const *dst, uint32_t *const **d_table) {
    const size_t polys = (size_t)bits * SELECT_BIT_POLYS, n_polys = q.n * polys;
    const size_t per_query = (q.form == FHS_SELECT_FORM_SEEDED ? polys / 2 : polys) * POLY_N;
    const size_t seed_words = q.form == FHS_SELECT_FORM_SEEDED ? q.n * 4 : 0, table_words = dst ? q.n : 0;
    const size_t total = q.n * per_query + seed_words + table_words;
    if (ctx.sel_query.cap < n_polys * 2 * POLY_N * 8) {
        hipError_t e = hipStreamSynchronize(ctx.stream);
        if (e == hipSuccess) e = ctx.sel_query.reserve(n_polys * 2 * POLY_N * 8);
        if (e != hipSuccess) return e;
    }
    if (!ctx.select_prepared) {
        if (hipError_t e = prepare_device_for_select()) return e;
        ctx.select_prepared = true;
    }
    size_t at = 0;
    if (!xfer_.ensure((total + BIG_CT) / (BIG_CT + 1), ctx.stream) || !xfer_.begin_table_pass(total, at, ctx.stream))
        return hipErrorOutOfMemory;
    uint64_t *pin = xfer_.pin() + at;
    for (size_t i = 0; i < q.n; i++) std::memcpy(pin + i * per_query, q.queries[i], per_query * 8);
    if (seed_words) std::memcpy(pin + q.n * per_query, q.seeds, seed_words * 8);
    if (table_words) std::memcpy(pin + q.n * per_query + seed_words, dst, table_words * 8);
    hipError_t e = xfer_.copy_up(at, total, ctx.stream);
    if (e != hipSuccess) return e;
    uint64_t *dev = xfer_.dev() + at;
    SelectQueryParams p{};
    p.words = dev;
    p.seeds = seed_words ? reinterpret_cast<const uint32_t *>(dev + q.n * per_query) : nullptr;
    p.n_polys = (uint32_t)n_polys; p.query_polys = (uint32_t)polys; p.quant_bits = BSK_QUANT_BITS;
    p.out = ctx.sel_query.as<double>(); p.tw = ctx.tw;
    if (d_table) *d_table = reinterpret_cast<uint32_t *const *>(dev + q.n * per_query + seed_words);
    return launch_select_query_to_ntt(p, ctx.stream);
}

// Then one launch per tree level and per rotate bit, every one over all q.n queries.  Launch k reads the entry (k = 0,
// every query the same words) or ctx.sel_ws[(k - 1) & 1] and writes ctx.sel_ws[k & 1] -- query y's nodes at y x (the
// level's nodes) GLWEs -- or, the last one, the destinations dst[y] = mask[2048] | body: never in place.  The three
// context buffers only grow, behind a drained stream (queued launches of an earlier select still read them).
hipError_t Engine::select_words(const SelectQueries &q, const uint32_t *d_mask, const uint32_t *d_body, size_t n_blocks,
                                const SelectShape &sh, uint32_t *const *dst) {
    const size_t ws_nodes[2] = {q.n * select_ws_nodes(sh, 0), q.n * select_ws_nodes(sh, 1)};
    const size_t glwe_bytes = (size_t)2 * POLY_N * sizeof(uint32_t);
    if (ctx.sel_ws[0].cap < ws_nodes[0] * glwe_bytes || ctx.sel_ws[1].cap < ws_nodes[1] * glwe_bytes) {
        hipError_t e = hipStreamSynchronize(ctx.stream);
        for (int k = 0; k < 2 && e == hipSuccess; k++) e = ctx.sel_ws[k].reserve(ws_nodes[k] * glwe_bytes);
        if (e != hipSuccess) return e;
    }
    uint32_t *const *d_table = nullptr;
    hipError_t e = select_queries_to_ntt(q, sh.bits, dst, &d_table);

    SelectCmuxParams p{};
    p.query_ntt = ctx.sel_query.as<double>(); p.tw = ctx.tw;
    p.queries = (uint32_t)q.n; p.query_stride = (size_t)sh.bits * SELECT_BIT_POLYS * 2 * POLY_N;
    p.src_mask = d_mask; p.src_body = d_body; p.src_nodes = (uint32_t)sh.groups; p.src_body_total = (uint32_t)n_blocks;
    p.src_stride = 0;
    const int launches = sh.tree_levels + sh.rot_bits;
    for (int k = 0; k < launches && e == hipSuccess; k++) {
        const bool tree = k < sh.tree_levels, last = k == launches - 1;
        const uint32_t out_nodes = tree ? (p.src_nodes + 1) / 2 : 1u;
        p.bit = tree ? sh.rot_bits + k : k - sh.tree_levels;
        p.rotate = tree ? 0u : (uint32_t)(sh.row_blocks << p.bit);
        p.dst_table = last ? d_table : nullptr;
        p.dst_mask = last ? nullptr : ctx.sel_ws[k & 1].as<uint32_t>();
        p.dst_body = last ? nullptr : p.dst_mask + (size_t)out_nodes * POLY_N;
        p.dst_stride = last ? 0 : (size_t)out_nodes * 2 * POLY_N;
        p.store_body = last ? (uint32_t)sh.row_blocks : (uint32_t)SELECT_GROUP;
        e = launch_select_cmux(p, ctx.stream);
        p.src_mask = p.dst_mask; p.src_body = p.dst_body; p.src_stride = p.dst_stride;
        p.src_nodes = out_nodes; p.src_body_total = out_nodes * SELECT_GROUP;
    }
    return e;
}

size_t Engine::select_batch_bytes(size_t n_chars, size_t row_chars, size_t n) {
    SelectShape sh;
    if (n == 0 || n > (size_t)FHS_SELECT_MAX_BATCH || !select_shape(n_chars, row_chars, sh)) return 0;
    return n * ((size_t)sh.bits * SELECT_BIT_POLYS * 2 * POLY_N * sizeof(double) +
                (select_ws_nodes(sh, 0) + select_ws_nodes(sh, 1)) * 2 * POLY_N * sizeof(uint32_t));
}

int Engine::store_select(uint64_t id, size_t row_chars, const SelectQueries &q, int bits, bool batch, uint64_t *ids_out) {
    auto it = store_.find(id);
    if (it == store_.end()) return ctx.fail(-1, "string store: unknown entry id");
    const StoreEntry &src = it->second;
    SelectShape sh;
    if ((src.n_blocks & 3) || !select_shape(src.n_blocks / 4, row_chars, sh))
        return ctx.fail(-1, "string store: select needs rows of a power of two of 1..512 characters, a whole number of them, at least two");
    if (bits != sh.bits) return ctx.fail(-1, "string store: the query's bit count is not fhs_store_select_bits of this shape");
    if (q.n == 0 || q.n > (size_t)FHS_SELECT_MAX_BATCH) return ctx.fail(-1, "string store: a batch is 1..FHS_SELECT_MAX_BATCH queries");
    if (!planner && !ctx.d_tables)
        return ctx.fail(-3, "string store: select needs the transform tables that the first fhs_load_server_key uploads");
    const int rekeys = src.rekeys + SELECT_REKEY_COST * (sh.tree_levels + sh.rot_bits);
    if (rekeys > STORE_MAX_REKEYS)
        return ctx.fail(-4, "string store: the selected entry would exceed FHS_STORE_MAX_REKEYS re-keys' worth of noise");
    if (batch && select_batch_bytes(src.n_blocks / 4, row_chars, q.n) > FHS_SELECT_BATCH_MAX_BYTES)
        return ctx.fail(-4, "string store: the batch's workspace would exceed FHS_SELECT_BATCH_MAX_BYTES");
    // block j of a result: the maxima over block j of every row; one fresh rotation group if any candidate has one
    std::vector<StoreEntry> dst(q.n);
    StoreEntry &first = dst[0];
    first.n_blocks = sh.row_blocks;
    first.var.assign(sh.row_blocks, 1); first.cycles.assign(sh.row_blocks, 0); first.rot.assign(sh.row_blocks, 0);
    first.rekeys = (uint8_t)rekeys;
    std::vector<uint8_t> grouped(sh.row_blocks, 0);
    bool any = false;
    for (size_t row = 0; row < sh.rows; row++)
        for (size_t j = 0; j < sh.row_blocks; j++) {
            const size_t t = row * sh.row_blocks + j;
            first.var[j] = std::max(first.var[j], src.var[t]);
            first.cycles[j] = std::max(first.cycles[j], src.cycles[t]);
            if (src.rot[t]) grouped[j] = 1, any = true;
        }
    for (size_t i = 1; i < q.n; i++) {
        dst[i].n_blocks = first.n_blocks; dst[i].var = first.var; dst[i].cycles = first.cycles; dst[i].rot = first.rot;
        dst[i].rekeys = first.rekeys;
    }
    if (!planner) {
        (void)hipSetDevice(ctx.device);
        hipError_t e = hipSuccess;
        std::vector<uint32_t *> out(q.n);
        for (size_t i = 0; i < q.n && e == hipSuccess; i++) {
            e = dst[i].buf.reserve_exact(dst[i].bytes());
            out[i] = dst[i].buf.as<uint32_t>();
        }
        if (e == hipSuccess)
            e = select_words(q, src.buf.as<uint32_t>(), src.buf.as<uint32_t>() + src.groups() * POLY_N, src.n_blocks, sh, out.data());
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx.stream);                  // before the new buffers go: a launch may be queued
            return ctx.hip_fail(e, "string store: select");
        }
    }
    for (size_t i = 0; i < q.n; i++) {
        if (any) {                                                   // every result its own group: they are not correlated
            const uint32_t fresh = ++rot_counter_ ? rot_counter_ : ++rot_counter_;
            for (size_t j = 0; j < sh.row_blocks; j++)
                if (grouped[j]) dst[i].rot[j] = fresh;
        }
        const uint64_t nid = ++store_ids_;
        store_.emplace(nid, std::move(dst[i]));
        ids_out[i] = nid;
    }
    return 0;
}

// Diagnostic: the same launches on raw host words, through a scratch allocation of the entry layout.
int Engine::debug_select(const SelectQueries &q, int bits, const uint32_t *mask32, const uint32_t *body32, size_t n_blocks,
                         size_t row_chars, uint32_t *mask_out, uint32_t *body_out) {
    if (planner) return ctx.fail(-3, "planner context: nothing is computed");
    SelectShape sh;
    if ((n_blocks & 3) || !select_shape(n_blocks / 4, row_chars, sh) || bits != sh.bits || q.n != 1)
        return ctx.fail(-1, "select (diagnostic): a refused shape or bit count");
    if (!ctx.d_tables) return ctx.fail(-3, "select needs the transform tables that the first fhs_load_server_key uploads");
    (void)hipSetDevice(ctx.device);
    const size_t mask_words = sh.groups * POLY_N;
    DevBuf buf;
    hipError_t e = buf.reserve_exact((mask_words + n_blocks + POLY_N + sh.row_blocks) * 4);
    uint32_t *d_mask = buf.as<uint32_t>(), *d_body = d_mask + mask_words, *d_mask_out = d_body + n_blocks, *d_body_out = d_mask_out + POLY_N;
    if (e == hipSuccess) e = hipMemcpyAsync(d_mask, mask32, mask_words * 4, hipMemcpyHostToDevice, ctx.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_body, body32, n_blocks * 4, hipMemcpyHostToDevice, ctx.stream);
    if (e == hipSuccess) e = select_words(q, d_mask, d_body, n_blocks, sh, &d_mask_out);
    if (e == hipSuccess) e = hipMemcpyAsync(mask_out, d_mask_out, POLY_N * 4, hipMemcpyDeviceToHost, ctx.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(body_out, d_body_out, sh.row_blocks * 4, hipMemcpyDeviceToHost, ctx.stream);
    hipError_t es = hipStreamSynchronize(ctx.stream);            // before buf goes, on every path
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return ctx.hip_fail(e, "select (diagnostic)");
    return 0;
}

// Diagnostic: the conversion kernel alone, out[bits][8][2 primes][2048] doubles.
int Engine::debug_select_query(const SelectQueries &q, int bits, double *out) {
    if (planner) return ctx.fail(-3, "planner context: nothing is computed");
    if (bits < 1 || bits > 24 || q.n != 1) return ctx.fail(-1, "select query (diagnostic): 1..24 bits");
    if (!ctx.d_tables) return ctx.fail(-3, "select needs the transform tables that the first fhs_load_server_key uploads");
    (void)hipSetDevice(ctx.device);
    const size_t bytes = (size_t)bits * SELECT_BIT_POLYS * 2 * POLY_N * sizeof(double);
    hipError_t e = select_queries_to_ntt(q, bits, nullptr, nullptr);
    if (e == hipSuccess) e = hipMemcpyAsync(out, ctx.sel_query.ptr, bytes, hipMemcpyDeviceToHost, ctx.stream);
    hipError_t es = hipStreamSynchronize(ctx.stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return ctx.hip_fail(e, "select query (diagnostic)");
    return 0;
}

// ---- block pool: trim ---------------------------------------------------------------------------------------------------
// After a flush every scheduled tick is in the stream: sched_ is empty, the ticks' accumulator-body blocks are back in
// the pool and nothing waits in free_after_, so the ONLY owners of pool pointers are the `dev` of the MAT nodes (checked
// below: their number is the pool's live count).  Levels waiting in planned_ hold more (out / body / term pointers): the
// call is refused while they exist, before the flush, which in capture mode would discard them.
int Engine::pool_trim(bool compact, size_t keep_free_blocks, uint64_t *blocks_moved, uint64_t *bytes_released) {
    if (blocks_moved) *blocks_moved = 0;
    if (bytes_released) *bytes_released = 0;
    if (!planned_.empty())
        return ctx.fail(-3, "block pool: levels planned by fhs_flush_plan are waiting for fhs_flush_level_commit");
    if (planner) return flush();
    (void)hipSetDevice(ctx.device);
    if (int rc = flush()) return rc;
    pool_.tick_enqueued(last_sched_tick_);                           // (nothing is scheduled any more)
    const size_t C = pool_.n_chunks(), CB = BlockPool::CHUNK_BLOCKS;
    if (C == 0) return 0;
    std::vector<Bid> owner;
    std::vector<uint64_t *> ptr;
    for (Bid id = 1; id < nodes_.size(); id++)
        if (nodes_[id].kind == BlockNode::MAT && nodes_[id].dev) { owner.push_back(id); ptr.push_back(nodes_[id].dev); }
    std::vector<uint32_t> chunk(ptr.size()), slot(ptr.size());
    uint64_t st[6];
    pool_.stats(st);
    if (ptr.size() != pool_.live() || st[4] != 0 || !pool_.locate(ptr.data(), ptr.size(), chunk.data(), slot.data()))
        return ctx.fail(-3, "internal: the node table does not own every live pool block after a flush");
    std::vector<uint32_t> live_per_chunk(C, 0);
    std::vector<uint8_t> used(C * CB, 0), victim(C, 0);
    for (size_t k = 0; k < ptr.size(); k++) { live_per_chunk[chunk[k]]++; used[chunk[k] * CB + slot[k]] = 1; }
    BlockPool::plan_trim(live_per_chunk.data(), C, keep_free_blocks, victim.data());
    if (!compact)
        for (size_t c = 0; c < C; c++)
            if (live_per_chunk[c]) victim[c] = 0;
    if (std::find(victim.begin(), victim.end(), 1) == victim.end()) return 0;
    // The moves.  Sources are live slots of victims, destinations free slots of kept chunks, first fit in chunk and slot
    // order: the two sets are disjoint and every destination is taken once, so neither the order of the rows inside a
    // launch nor that of the launches matters.  The kept chunks have room: 2048 K >= live + keep_free_blocks.
    std::vector<size_t> moving;                                      // indices into owner / ptr
    for (size_t k = 0; k < ptr.size(); k++)
        if (victim[chunk[k]]) moving.push_back(k);
    std::vector<uint64_t *> dest(moving.size());
    {
        size_t at = 0;
        for (size_t m = 0; m < moving.size(); m++) {
            while (at < C * CB && (victim[at / CB] || used[at])) at++;
            if (at == C * CB) return ctx.fail(-3, "internal: block pool: no free slot for a moved block");
            used[at] = 1;
            dest[m] = pool_.slot_ptr(at / CB, at % CB);
        }
    }
    for (size_t done = 0, n; done < moving.size(); done += n) {
        n = std::min(POOL_MOVE_MAX_BATCH, moving.size() - done);
        size_t at = 0;
        if (!xfer_.begin_table_pass(2 * n, at, ctx.stream)) return ctx.fail(-2, "block pool: no transfer buffer for the move tables");
        uint64_t *tab = xfer_.pin() + at;
        for (size_t k = 0; k < n; k++) {
            tab[k] = (uint64_t)(uintptr_t)ptr[moving[done + k]];
            tab[n + k] = (uint64_t)(uintptr_t)dest[done + k];
        }
        hipError_t e = xfer_.copy_up(at, 2 * n, ctx.stream);
        if (e == hipSuccess)
            e = launch_pool_move_blocks(reinterpret_cast<const uint64_t *const *>(xfer_.dev() + at),
                                        reinterpret_cast<uint64_t *const *>(xfer_.dev() + at + n), (int)n, ctx.stream);
        if (e != hipSuccess) {                                       // nothing was rewritten: the copies made so far are
            (void)hipStreamSynchronize(ctx.stream);                  // garbage in free slots
            return ctx.hip_fail(e, "block pool: move");
        }
    }
    // in this order: the stream has finished (the moves, and every queued reader of a victim), the nodes point at the
    // copies, the free list forgets the victims' slots and the destinations, the victims' allocations go
    hipError_t e = hipStreamSynchronize(ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "block pool: trim");
    for (size_t m = 0; m < moving.size(); m++) nodes_[owner[moving[m]]].dev = dest[m];
    const uint64_t bytes = pool_.release(victim, used);
    if (blocks_moved) *blocks_moved = moving.size();
    if (bytes_released) *bytes_released = bytes;
    return 0;
}

int Engine::copy_block_to_device(Bid b, uint64_t *d_out, bool wait, bool do_flush) {
    if (planner) return ctx.fail(-3, "planner context: nothing is computed");
    (void)hipSetDevice(ctx.device);
    int rc = do_flush ? flush() : 0;
    if (rc) return rc;
    hipError_t e;
    if (nodes_[b].kind == BlockNode::TRIV) {
        // body = triv << 59: only its high word is non-zero, written by a 32-bit memset (no host buffer in flight)
        const uint64_t body = (uint64_t)nodes_[b].triv << DELTA_LOG;
        e = hipMemsetAsync(d_out, 0, BIG_CT * 8, ctx.stream);
        if (e == hipSuccess)
            e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reinterpret_cast<uint32_t *>(d_out + BIG_N) + 1),
                                  (int)(uint32_t)(body >> 32), 1, ctx.stream);
    } else {
        if (nodes_[b].kind == BlockNode::LIN && (rc = materialize_lin(b))) return rc;
        if (nodes_[b].kind != BlockNode::MAT) return ctx.fail(-3, "internal: block not materialised");
        e = hipMemcpyAsync(d_out, nodes_[b].dev, BIG_CT * 8, hipMemcpyDeviceToDevice, ctx.stream);
    }
    if (e == hipSuccess && wait) e = hipStreamSynchronize(ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "export");
    return 0;
}

uint64_t Engine::new_char(const Bid b[4]) {
    uint64_t h;
    if (!free_chars_.empty()) {
        h = free_chars_.back();
        free_chars_.pop_back();
    } else {
        chars_.emplace_back();
        h = chars_.size();
    }
    CharRec &c = chars_[h - 1];
    for (int i = 0; i < 4; i++) c.b[i] = b[i];
    c.used = true;
    return h;
}

void Engine::free_char(uint64_t h) {
    CharRec &c = chars_[h - 1];
    for (int i = 0; i < 4; i++) release(c.b[i]);
    c.used = false;
    free_chars_.push_back(h);
}

}  // namespace fhs
