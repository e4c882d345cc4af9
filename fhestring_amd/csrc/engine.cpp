#include "engine.h"
#include "../../include/fhestring_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

namespace fhs {

int Engine::on_key_loaded() {
    if (!d_luts_) {
        std::vector<uint64_t> host((size_t)LUT_COUNT * POLY_N);
        for (int id = 0; id < LUT_COUNT; id++) make_lut_poly(id, host.data() + (size_t)id * POLY_N);
        luts_clean_ = Context::luts_low_bytes_clear(host.data(), host.size());
        hipError_t e = d_luts_.reserve_exact(host.size() * 8);
        if (e != hipSuccess) return ctx.hip_fail(e, "hipMalloc luts");
        e = hipMemcpy(d_luts_.ptr, host.data(), host.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) return ctx.hip_fail(e, "copy luts");
    }
    return 0;
}

// The user tables among ids[n] that this context has not used yet get the next slots of the device array and are expanded
// there on the context's stream (expand_user_luts_kernel: only the 16-byte descriptors cross the bus), in front of the
// launch group that names them.  An array that has to grow waits for the stream first -- queued launch groups read the
// old one -- and takes its contents along; it doubles, so a context pays that wait a handful of times in its life.
int Engine::ensure_luts(const uint32_t *ids, size_t n) {
    std::vector<uint32_t> fresh;
    for (size_t k = 0; k < n; k++)
        if (ids[k] >= LUT_COUNT && !lut_slot_.count(ids[k]) && std::find(fresh.begin(), fresh.end(), ids[k]) == fresh.end())
            fresh.push_back(ids[k]);
    if (fresh.empty()) return 0;
    std::vector<uint8_t> desc(fresh.size() * 16);
    for (size_t k = 0; k < fresh.size(); k++) {
        const uint8_t *v = user_lut_values((int)fresh[k]);
        if (!v) return ctx.fail(-1, "look-up table id " + std::to_string(fresh[k]) + " is not registered");
        std::memcpy(&desc[16 * k], v, 16);
    }
    if (hipSetDevice(ctx.device) != hipSuccess) return ctx.fail(-2, "hipSetDevice failed");
    if (!d_luts_) return ctx.fail(-3, "server key not loaded");
    const size_t need = lut_slots_ + fresh.size();
    if (need > lut_cap_) {
        const size_t cap = std::max({need, 2 * lut_cap_, (size_t)LUT_COUNT + 64});
        DevBuf grown;
        hipError_t e = hipStreamSynchronize(ctx.stream);
        if (e == hipSuccess) e = grown.reserve_exact(cap * POLY_N * 8);
        if (e == hipSuccess) e = hipMemcpy(grown.ptr, d_luts_.ptr, lut_slots_ * POLY_N * 8, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return ctx.hip_fail(e, "growing the look-up table array");
        d_luts_ = std::move(grown);
        lut_cap_ = cap;
    }
    hipError_t e = launch_expand_user_luts(reinterpret_cast<const uint8_t(*)[16]>(desc.data()), (int)fresh.size(),
                                           d_luts_.as<uint64_t>() + lut_slots_ * POLY_N, ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "user table expansion launch");
    for (uint32_t id : fresh) lut_slot_[id] = (uint32_t)lut_slots_++;
    return 0;
}
int Engine::ensure_luts(const TickLevel *levels, size_t n_levels) {
    for (size_t j = 0; j < n_levels; j++)
        if (int rc = ensure_luts(levels[j].lut.data(), levels[j].lut.size())) return rc;
    return 0;
}

int Engine::read_lut(int lut_id, uint64_t *host_out) {
    if (planner) return ctx.fail(-3, "a planner context has no device tables");
    if (lut_id < 0 || (lut_id >= LUT_COUNT && !user_lut_values(lut_id))) return ctx.fail(-1, "unknown look-up table id");
    const uint32_t id = (uint32_t)lut_id;
    if (int rc = ensure_luts(&id, 1)) return rc;
    if (!d_luts_) return ctx.fail(-3, "server key not loaded");
    hipError_t e = hipStreamSynchronize(ctx.stream);
    if (e == hipSuccess)
        e = hipMemcpy(host_out, d_luts_.as<uint64_t>() + (size_t)lut_slot(id) * POLY_N, POLY_N * 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : ctx.hip_fail(e, "table download");
}

Engine::~Engine() {
    if (!planner && ctx.stream) (void)hipStreamSynchronize(ctx.stream);
}

bool BlockPool::grow() {
    DevBuf c;
    if (c.reserve_exact(CHUNK_BLOCKS * STRIDE * 8) != hipSuccess) return false;
    uint64_t *base = c.as<uint64_t>();
    for (size_t i = CHUNK_BLOCKS; i-- > 0;) free_.push_back(base + i * STRIDE);
    chunks_.push_back(std::move(c));
    return true;
}
void BlockPool::tick_enqueued(uint64_t tick) {
    while (!free_after_.empty() && free_after_.begin()->first <= tick) {
        for (uint64_t *p : free_after_.begin()->second) free_.push_back(p);
        free_after_.erase(free_after_.begin());
    }
}

void BlockPool::stats(uint64_t out[6]) const {
    uint64_t waiting = 0;
    for (const auto &kv : free_after_) waiting += kv.second.size();
    out[0] = chunks_.size();
    out[1] = CHUNK_BLOCKS;
    out[2] = live_;
    out[3] = free_.size();
    out[4] = waiting;
    out[5] = chunks_.size() * CHUNK_BYTES;
}

void BlockPool::plan_trim(const uint32_t *live_per_chunk, size_t n_chunks, size_t keep_free_blocks, uint8_t *victim) {
    uint64_t live = 0;
    for (size_t i = 0; i < n_chunks; i++) { live += live_per_chunk[i]; victim[i] = 0; }
    // (a reserve beyond what the chunks could hold keeps them all: no sum that could wrap)
    if (keep_free_blocks >= n_chunks * CHUNK_BLOCKS) return;
    const size_t keep = (size_t)((live + keep_free_blocks + CHUNK_BLOCKS - 1) / CHUNK_BLOCKS);
    if (keep >= n_chunks) return;
    std::vector<uint32_t> order(n_chunks);
    for (size_t i = 0; i < n_chunks; i++) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return live_per_chunk[a] != live_per_chunk[b] ? live_per_chunk[a] < live_per_chunk[b] : a > b;
    });
    for (size_t k = 0; k < n_chunks - keep; k++) victim[order[k]] = 1;
}

bool BlockPool::locate(uint64_t *const *p, size_t n, uint32_t *chunk, uint32_t *slot) const {
    std::vector<std::pair<uintptr_t, uint32_t>> bases(chunks_.size());   // the chunks by address
    for (size_t i = 0; i < chunks_.size(); i++) bases[i] = {(uintptr_t)chunks_[i].ptr, (uint32_t)i};
    std::sort(bases.begin(), bases.end());
    for (size_t k = 0; k < n; k++) {
        const uintptr_t a = (uintptr_t)p[k];
        auto it = std::upper_bound(bases.begin(), bases.end(), std::make_pair(a, ~(uint32_t)0));
        if (it == bases.begin()) return false;
        --it;
        const uintptr_t off = a - it->first;
        if (off >= CHUNK_BYTES || off % (STRIDE * 8)) return false;
        chunk[k] = it->second;
        slot[k] = (uint32_t)(off / (STRIDE * 8));
    }
    return true;
}

uint64_t BlockPool::release(const std::vector<uint8_t> &victim, const std::vector<uint8_t> &used) {
    std::vector<uint32_t> chunk(free_.size()), slot(free_.size());
    if (!locate(free_.data(), free_.size(), chunk.data(), slot.data())) return 0;
    size_t kept = 0;
    for (size_t k = 0; k < free_.size(); k++)
        if (!victim[chunk[k]] && !used[chunk[k] * CHUNK_BLOCKS + slot[k]]) free_[kept++] = free_[k];
    free_.resize(kept);
    uint64_t bytes = 0;
    std::vector<DevBuf> rest;
    for (size_t i = 0; i < chunks_.size(); i++) {
        if (victim[i]) bytes += CHUNK_BYTES;                  // (its DevBuf dies with the old vector)
        else rest.push_back(std::move(chunks_[i]));
    }
    chunks_.swap(rest);
    return bytes;
}

Bid Engine::new_node() {
    Bid id;
    if (!free_nodes_.empty()) {
        id = free_nodes_.back();
        free_nodes_.pop_back();
    } else {
        id = (Bid)nodes_.size();
        nodes_.emplace_back();
    }
    BlockNode &n = nodes_[id];
    const uint32_t g = n.gen + 1;
    n = BlockNode();
    n.gen = g;
    n.refs = 1;
    return id;
}

void Engine::retain(Bid b) { nodes_[b].refs++; }

void Engine::release(Bid b) {
    if (nodes_[b].refs > 1) {                                 // the common case: no heap traffic, nothing dies
        nodes_[b].refs--;
        return;
    }
    // iterative: chains of pending nodes can be tens of thousands deep (as-written `len`)
    std::vector<Bid> stack{b};
    while (!stack.empty()) {
        Bid id = stack.back();
        stack.pop_back();
        BlockNode &n = nodes_[id];
        if (--n.refs > 0) continue;
        if (n.kind == BlockNode::MAT && n.dev) free_block(n.dev);
        if (n.kind == BlockNode::PBS && n.src) stack.push_back(n.src);
        if (n.kind == BlockNode::LIN)
            for (const Term &t : n.terms) stack.push_back(t.blk);
        n.terms.clear();
        n.terms.shrink_to_fit();
        n.kind = BlockNode::FREE;
        n.dev = nullptr;
        n.src = 0;
        free_nodes_.push_back(id);
    }
}

Bid Engine::triv(int v) {
    Bid id = new_node();
    nodes_[id].kind = BlockNode::TRIV;
    nodes_[id].triv = (uint8_t)(v & 31);
    return id;
}

// sum(coef*blk) + konst.  Trivial terms fold into the constant, nested LINs are flattened and
// duplicate blocks merged, so a LIN only ever refers to MAT or PBS nodes.
Bid Engine::lin(const Term *terms, size_t n, int konst) {
    int64_t k = konst;
    std::vector<Term> flat;
    auto add = [&](int64_t c, Bid b) {
        if (c == 0) return;
        for (Term &t : flat)
            if (t.blk == b) { t.coef += c; return; }
        flat.push_back({c, b});
    };
    for (size_t i = 0; i < n; i++) {
        const int64_t c = terms[i].coef;
        const BlockNode &s = nodes_[terms[i].blk];
        if (c == 0) continue;
        if (s.kind == BlockNode::TRIV) k += c * s.triv;
        else if (s.kind == BlockNode::LIN) {
            k += c * s.konst;
            for (const Term &t : s.terms) add(c * t.coef, t.blk);
        } else add(c, terms[i].blk);
    }
    flat.erase(std::remove_if(flat.begin(), flat.end(), [](const Term &t) { return t.coef == 0; }), flat.end());
    if (flat.empty()) return triv((int)(((k % 32) + 32) % 32));
    if (flat.size() == 1 && flat[0].coef == 1 && (((k % 32) + 32) % 32) == 0) {
        retain(flat[0].blk);   // identity: share the block
        return flat[0].blk;
    }
    Bid id = new_node();
    uint32_t lvl = 0;
    for (const Term &t : flat) {
        retain(t.blk);
        lvl = std::max(lvl, nodes_[t.blk].level);
    }
    BlockNode &nn = nodes_[id];
    nn.kind = BlockNode::LIN;
    nn.konst = (int32_t)(((k % 32) + 32) % 32);
    nn.level = lvl;
    nn.terms = std::move(flat);
    return id;
}

void Engine::describe_block(Bid b, std::vector<uint64_t> &out) const {
    const BlockNode &n = nodes_[b];
    if (n.kind == BlockNode::TRIV) { out.insert(out.end(), {0, (uint64_t)(triv_val(b) & 31), 0}); return; }
    if (n.kind == BlockNode::MAT) { out.insert(out.end(), {1, 0, 1, (uint64_t)(uintptr_t)n.dev, 1}); return; }
    if (n.kind != BlockNode::LIN) { out.insert(out.end(), {3, 0, 0}); return; }
    out.insert(out.end(), {2, (uint64_t)(n.konst & 31), (uint64_t)n.terms.size()});
    for (const Term &t : n.terms) {
        const BlockNode &tb = nodes_[t.blk];
        out.push_back(tb.kind == BlockNode::MAT ? (uint64_t)(uintptr_t)tb.dev : 0);
        out.push_back((uint64_t)t.coef);
    }
}

int64_t Engine::sum_c2(Bid b) const {
    const BlockNode &n = nodes_[b];
    if (n.kind == BlockNode::TRIV) return 0;
    if (n.kind == BlockNode::MAT) return n.var;
    if (n.kind != BlockNode::LIN) return 1;
    return lin_c2(n.terms);
}

int64_t Engine::lin_c2(const std::vector<Term> &terms) const {
    // var(sum c_i e_i) = sum c_i^2 var_i + 2 sum_{i<j} rho_ij c_i c_j sqrt(var_i var_j) over extractions of ONE rotation.
    // Measured on the MI355X (profiles/r05_rotation_sharing_rho.txt, tools/rho_profile.py): rho falls linearly with the
    // constant difference dt from +0.45 (dt -> 0) through 0 (dt = 8) to -0.45 (dt = 15) -- the decomposition-rounding error
    // reaches every coefficient through the negacyclic product with the binary GLWE key -- and is exactly -1 at dt = 16
    // (the same coefficient negated: such rows never share).  The measurement is per key and per sample (max |rho| 0.48
    // +- 0.03 on one key, profiles/r06_margins.json repeats it on three), so the bookkeeping does not rest on it: a group
    // is charged as FULLY correlated, |rho| <= 1, which Cauchy-Schwarz proves whatever the key and the signs:
    //     group cost = (sum |c|)^2   (>= sum c^2 + 2 sum_{i<j} rho_ij c_i c_j for every |rho_ij| <= 1).
    int64_t c2 = 0;
    struct Grp { uint32_t rot; int64_t sum_abs, sum_c2, var; };
    Grp grp[8];
    int ng = 0;
    for (const Term &t : terms) {
        const BlockNode &tb = nodes_[t.blk];
        const int64_t var = tb.kind == BlockNode::MAT ? tb.var : 1;
        if (tb.kind != BlockNode::MAT || tb.rot == 0) { c2 += t.coef * t.coef * var; continue; }
        int g = 0;
        while (g < ng && grp[g].rot != tb.rot) g++;
        if (g == ng) {
            if (ng == 8) { c2 += t.coef * t.coef * var; continue; }       // (more than 8 shared rotations in one sum: unseen)
            grp[ng++] = Grp{tb.rot, 0, 0, 0};
        }
        grp[g].sum_abs += t.coef < 0 ? -t.coef : t.coef;
        grp[g].sum_c2 += t.coef * t.coef;
        grp[g].var = std::max(grp[g].var, var);
    }
    for (int g = 0; g < ng; g++)
        c2 += grp[g].sum_abs * grp[g].sum_abs * grp[g].var;
    return c2;
}

int Engine::set_var(Bid b, uint64_t v, bool check_only) {
    BlockNode &n = nodes_[b];
    if (n.kind == BlockNode::TRIV) return 0;                  // a plaintext block carries no noise whatever is declared
    if (n.kind != BlockNode::MAT) return ctx.fail(-1, "noise can only be declared for uploaded ciphertexts");
    // a declaration can only ADD to what the bookkeeping knows: an upload starts at 1, a block the library itself
    // materialised from a sum keeps at least its own figure (no laundering through this entry point)
    if (v < n.var) return ctx.fail(-1, "fhs_char_set_noise: the declared figure is below the one the library tracks for this block");
    if (!check_only) n.var = (uint16_t)std::min<uint64_t>(std::max<uint64_t>(v, 1), 65535);
    return 0;
}

Bid Engine::pbs(Bid x, int lut) {
    const BlockNode &s = nodes_[x];
    if (s.kind == BlockNode::TRIV) {   // constant folding: no PBS is executed
        stats.pbs_folded++;
        return triv(lut_eval(lut, s.triv));
    }
    const uint32_t lvl = s.level + 1;
    // fused mode: an identical bootstrap (same LUT on the same linear combination of the same blocks) is computed once,
    // e.g. the high-nibble test of a character against pattern characters that share their high nibble
    uint64_t h1 = 0, h2 = 0, nk_hash = 0;
    const bool share = mode == 1;
    if (share) {
        auto mix = [](uint64_t v, uint64_t k) {
            v = (v ^ (v >> 31)) * k;
            v = (v ^ (v >> 29)) * 0xBF58476D1CE4E5B9ull;
            return v ^ (v >> 32);
        };
        auto term = [&](uint64_t blk, uint64_t gen, int64_t coef) {      // commutative: the order of terms is irrelevant
            const uint64_t v = (blk << 32 | gen) + 0x9E3779B97F4A7C15ull * (uint64_t)coef;
            h1 += mix(v, 0x94D049BB133111EBull);
            h2 += mix(v + 0x632BE59BD9B4E019ull, 0xD6E8FEB86659FD93ull);
        };
        if (s.kind == BlockNode::LIN) {
            for (const Term &t : s.terms) term(t.blk, nodes_[t.blk].gen, t.coef);
            nk_hash = mix(h1 ^ h2 ^ ((uint64_t)lut << 48), 0x9E3779B97F4A7C15ull) | 1;      // before the constant goes in
            h1 += mix((uint64_t)(uint32_t)s.konst + 77, 0x94D049BB133111EBull);
            h2 += mix((uint64_t)(uint32_t)s.konst + 131, 0xD6E8FEB86659FD93ull);
        } else {
            term(x, s.gen, 1);
            nk_hash = mix(h1 ^ h2 ^ ((uint64_t)lut << 48), 0x9E3779B97F4A7C15ull) | 1;
        }
        h1 = mix(h1 + (uint64_t)lut * 0x9E3779B97F4A7C15ull, 0xD6E8FEB86659FD93ull);
        h2 = mix(h2 ^ ((uint64_t)lut << 40), 0x94D049BB133111EBull);
        auto it = cse_.find(h1);
        if (it != cse_.end() && it->second.h2 == h2) {
            const Bid id = it->second.id;
            const BlockNode &c = nodes_[id];
            if (c.gen == it->second.gen && c.refs > 0 && (c.kind == BlockNode::PBS || c.kind == BlockNode::MAT)) {
                stats.pbs_shared++;
                retain(id);
                return id;
            }
        }
    }
    retain(x);
    Bid id = new_node();
    BlockNode &n = nodes_[id];
    n.kind = BlockNode::PBS;
    n.src = x;
    n.lut = (uint16_t)lut;
    n.level = lvl;
    n.nk = (share && share_rotations && !(level_parallel && ctx.dist.active())) ? nk_hash : 0;
    pending_.push_back({id, n.gen});
    if (lvl == 1) { n_depth1_++; depth1_add(n); }
    if (auto_flush_pending && !manual_jobs_ && !capture_max_rows && !in_auto_flush_ &&
        sched_.empty() && !(dist_world > 1 && !level_parallel) && (planner || ctx.key_loaded)) {
        // peel the ready level when a whole batch has accumulated -- or, on a real device, as soon as a grid's worth is
        // ready and the previous launch group has finished (polled every 256 recorded bootstraps): the GPU never idles
        // while the host is still recording, and nothing narrower than one full round of workgroups is launched early
        // (level-parallel ranks must all take the same decisions: there only the deterministic count rule applies)
        // counted in blind ROTATIONS: rows that will share one (rotation sharing) are one unit of GPU work
        const size_t ready = depth1_rotations();
        bool go = ready >= auto_flush_pending;
        peel_limit_ = 0;
        const size_t round = balance_slots ? balance_slots : 1024;
        if (!go && ready >= round && !planner && !level_parallel && last_group_done_.peek() && (++idle_poll_ & 255) == 0) {
            go = hipEventQuery(last_group_done_.peek()) == hipSuccess;
            // an idle GPU gets whole rounds of the persistent kernel only: 1 191 ready rows launched as they are cost two
            // rounds; the remainder stays pending (it is ready, and joins the next launch)
            peel_limit_ = ready / round * round;
        }
        if (go) {
            in_auto_flush_ = true;
            if (int rc = plan_job(true, true)) {              // kept: the caller's next flush reports THIS cause
                if (!auto_flush_rc_) { auto_flush_rc_ = rc; auto_flush_err_ = ctx.err; }
            }
            in_auto_flush_ = false;
        }
    }
    if (share) {
        if (cse_.empty()) cse_.reserve(1u << 18);
        if (cse_.size() > (1u << 21)) cse_.clear();           // bounded: stale entries are only dead weight
        cse_[h1] = CseEntry{h2, id, n.gen};
    }
    return id;
}

// ------------------------------------------------------------------------------------------
// flush: plan the pending levels one by one and enqueue each as soon as it is planned
// ------------------------------------------------------------------------------------------
int Engine::flush() {
    if (auto_flush_rc_) {                                     // an automatic partial flush failed while the DAG was recorded
        const int rc = auto_flush_rc_;
        auto_flush_rc_ = 0;
        return ctx.fail(rc, "automatic partial flush failed: " + auto_flush_err_);
    }
    while (!sched_.empty())                                   // drain the scheduled ticks of submitted jobs first
        if (int rc = pump(1)) return rc;
    if (level_parallel && ctx.dist.active()) return plan_job(true);   // world 1 too: same stream-ordered path
    if (dist_world > 1 && !pending_.empty())
        return ctx.fail(-3, "distributed context: pending PBS must be run with fhs_flush_plan/level_exec/level_commit");
    manual_jobs_ = false;                                     // every scheduled tick is in the stream: automatic partial flushes may resume
    const bool plan_capture = capture_max_rows && !capture_live;   // the all-at-once plan keeps the records (no sharing)
    if (!plan_capture && balance_slots) {
        // round-aligned launch groups inside ONE operation as well: the levels go through the tick scheduler at row
        // granularity (plan_job), every tick is enqueued as soon as it is complete
        if (int rc = plan_job(false, false, true)) return rc;
        while (!sched_.empty())
            if (int rc = pump(1)) return rc;
        return 0;
    }
    if (!plan_capture) return plan_job(true);                 // level by level: planning overlaps execution
    int rc = plan_flush();                                    // capture mode: unshared, whole levels, in level order
    if (rc) return rc;
    for (size_t k = 0; k < planned_.size(); k++)
        if ((rc = exec_level(k, 0, planned_[k].descs.size(), nullptr))) return rc;
    planned_.clear();
    return 0;
}

// ------------------------------------------------------------------------------------------
// the level builder: pending bootstraps -> levels -> rows (plan_job and plan_flush)
// ------------------------------------------------------------------------------------------
void Engine::reset_depth1() {
    n_depth1_ = 0;
    n_depth1_solo_ = 0;
    depth1_keys_.clear();
}

// pending_ -> the live pending bootstraps by level; first_level_only: depth 1 only (at most peel_limit_ rotations), the
// other pending nodes stay pending, one level shallower than before
Engine::LevelMap Engine::collect_levels(bool first_level_only) {
    LevelMap by_level;
    reset_depth1();
    if (!first_level_only) {
        for (const Pend &p : pending_)
            if (nodes_[p.id].kind == BlockNode::PBS && nodes_[p.id].gen == p.gen) by_level[nodes_[p.id].level].push_back(p.id);
        pending_.clear();
        return by_level;
    }
    std::vector<Pend> rest;
    const size_t limit = peel_limit_ ? peel_limit_ : ~(size_t)0;     // in ROTATIONS: rows sharing a taken row's key ride along
    size_t left_ready = 0, taken_rot = 0;
    std::unordered_map<uint64_t, char> taken_keys;
    for (const Pend &p : pending_) {
        BlockNode &n = nodes_[p.id];
        if (n.kind != BlockNode::PBS || n.gen != p.gen) continue;
        bool take = false;
        if (n.level <= 1) {
            if (n.nk && taken_keys.count(n.nk)) take = true;
            else if (taken_rot < limit) {
                take = true;
                taken_rot++;
                if (n.nk) taken_keys[n.nk] = 1;
            }
        }
        if (take) by_level[1].push_back(p.id);
        else {
            if (n.level <= 1) { left_ready++; depth1_add(n); }
            rest.push_back(p);
        }
    }
    // every ready row taken: the rest moves one level up.  A partial peel (whole rounds only) leaves the levels alone:
    // a stale level is only ever too HIGH, which keeps the order valid
    if (left_ready == 0) {
        for (const Pend &p : rest)
            if (--nodes_[p.id].level == 1) { n_depth1_++; depth1_add(nodes_[p.id]); }
    } else {
        n_depth1_ = left_ready;
    }
    peel_limit_ = 0;
    pending_.swap(rest);
    return by_level;
}

// ---- rotation sharing ----------------------------------------------------------------------------------------------
// Rows of this level with the same look-up table on the same linear combination up to its trivial CONSTANT
// (e.g. the nibble of a character tested against the different nibbles of a clear pattern: is0(x - c)) share ONE
// keyswitch + blind rotation: adding c * Delta to a ciphertext rotates the accumulator by X^(128 c) exactly, so the
// other rows are further sample extractions of the leader's accumulator (extract_shift_kernel) -- the same
// ciphertext a bootstrap of their own would give, up to decomposition ties (the CPU oracle restates it:
// orc_pbs_shifted).  The level is reordered: rotation rows first (their number is returned), followers behind.
size_t Engine::share_level(LevelMap &by_level, LevelMap::iterator lvit, bool first_level_only, std::vector<ShareRow> &followers) {
    std::vector<Bid> &lv = lvit->second;
    followers.clear();
    if (!(share_rotations && mode == 1 && lv.size() > 1 && !(level_parallel && ctx.dist.active()))) return lv.size();
    std::unordered_map<uint64_t, std::vector<uint32_t>> seen;     // hash of (lut, terms) -> leader positions
    std::vector<Bid> rot, fol;
    std::vector<ShareRow> fmeta;
    std::vector<uint32_t> used;                                    // per rotation row: bit t = an extraction at shift t exists
    auto key_terms = [&](const BlockNode &src, Bid self, std::vector<std::pair<Bid, int64_t>> &tt, int &konst) {
        tt.clear();
        if (src.kind == BlockNode::LIN) {
            for (const Term &t : src.terms) tt.emplace_back(t.blk, t.coef);
            std::sort(tt.begin(), tt.end());
            konst = src.konst;
        } else {
            tt.emplace_back(self, 1);
            konst = 0;
        }
    };
    std::vector<std::pair<Bid, int64_t>> ta, tb;
    for (Bid b : lv) {
        const BlockNode &n = nodes_[b];
        int ka = 0;
        key_terms(nodes_[n.src], n.src, ta, ka);
        uint64_t h = 0x9E3779B97F4A7C15ull * (uint64_t)(n.lut + 1);
        for (auto &t : ta) {
            h ^= ((uint64_t)t.first << 20) + (uint64_t)t.second * 0xBF58476D1CE4E5B9ull;
            h = (h ^ (h >> 29)) * 0x94D049BB133111EBull;
        }
        std::vector<uint32_t> &cand = seen[h];
        bool shared = false;
        for (uint32_t pos : cand) {
            const BlockNode &ln = nodes_[rot[pos]];
            int kb = 0;
            key_terms(nodes_[ln.src], ln.src, tb, kb);
            if (ln.lut != n.lut || ta != tb) continue;
            // a constant difference of 16 is the SAME coefficient of the accumulator, negated (X^2048 = -1): its
            // error is exactly minus the other's (rho = -1; the full-correlation charge of lin_c2 covers it, but a
            // sum a - b of the two would DOUBLE the error for no information) -- no two members of a group may be
            // 16 apart (such a row joins another group of the same key, or starts one)
            const uint32_t t = (uint32_t)(((ka - kb) % 32 + 32) % 32);
            if (used[pos] & (1u << ((t + 16) & 31))) continue;
            used[pos] |= 1u << t;
            fol.push_back(b);
            fmeta.push_back({pos, 128 * t, nullptr});
            shared = true;
            break;
        }
        if (!shared) {
            cand.push_back((uint32_t)rot.size());
            rot.push_back(b);
            used.push_back(1u);                                    // the leader itself: shift 0
        }
    }
    if (!fol.empty()) unshare_over_budget(by_level, lvit, first_level_only, rot, fol, fmeta);
    if (fol.empty()) return lv.size();
    const size_t R = rot.size();
    lv.swap(rot);
    lv.insert(lv.end(), fol.begin(), fol.end());
    followers.swap(fmeta);
    return R;
}

// Sharing must not push a CONSUMER over the noise budget: extractions of one rotation are correlated (lin_c2 charges
// them as fully correlated), so a later bootstrap whose input sums several members of one group with the same sign is
// charged cross terms the string layer did not see when it built that sum.  Every pending consumer is known here
// (deeper levels of this plan; in a partial peel the nodes still pending) -- consumers recorded later see the groups
// through sum_c2().  A follower whose group would take a consumer from within the budget to beyond it gets a rotation
// of its own (appended to `rot`: positions stay valid).
void Engine::unshare_over_budget(const LevelMap &by_level, LevelMap::const_iterator lvit, bool first_level_only,
                                 std::vector<Bid> &rot, std::vector<Bid> &fol, std::vector<ShareRow> &fmeta) {
    std::unordered_map<Bid, uint32_t> member;              // node -> leader position (leaders with followers too)
    for (size_t i = 0; i < fol.size(); i++) {
        member[fol[i]] = fmeta[i].lead_row;
        member[rot[fmeta[i].lead_row]] = fmeta[i].lead_row;
    }
    std::vector<char> unshare(fol.size(), 0);
    bool any_unshare = false;
    auto check = [&](Bid consumer) {
        const BlockNode &cn = nodes_[consumer];
        if (cn.kind != BlockNode::PBS) return;
        const BlockNode &src = nodes_[cn.src];
        if (src.kind != BlockNode::LIN || src.terms.size() < 2) return;
        struct G { uint32_t lead; int64_t sum_abs, sum_c2; };
        G g[8];
        int ng = 0;
        bool multi = false;
        for (const Term &t : src.terms) {
            auto it = member.find(t.blk);
            if (it == member.end()) continue;
            int k = 0;
            while (k < ng && g[k].lead != it->second) k++;
            if (k == ng) { if (ng == 8) continue; g[ng++] = G{it->second, 0, 0}; }
            else multi = true;
            g[k].sum_abs += t.coef < 0 ? -t.coef : t.coef;
            g[k].sum_c2 += t.coef * t.coef;
        }
        if (!multi) return;
        int64_t plain = lin_c2(src.terms), extra = 0;      // (members are still pending: counted as independent)
        for (int k = 0; k < ng; k++) extra += g[k].sum_abs * g[k].sum_abs - g[k].sum_c2;   // as lin_c2 will
        if (plain + extra <= FHS_NOISE_BUDGET_SUM_C2 || extra == 0) return;
        for (const Term &t : src.terms)                    // the followers among this sum's terms leave their groups
            for (size_t i = 0; i < fol.size(); i++)
                if (fol[i] == t.blk && !unshare[i]) { unshare[i] = 1; any_unshare = true; }
    };
    for (auto nx = std::next(lvit); nx != by_level.end(); ++nx)
        for (Bid c : nx->second) check(c);
    if (first_level_only)
        for (const Pend &pd : pending_)
            if (nodes_[pd.id].gen == pd.gen) check(pd.id);
    if (!any_unshare) return;
    std::vector<Bid> fol2;
    std::vector<ShareRow> fmeta2;
    for (size_t i = 0; i < fol.size(); i++) {
        if (unshare[i]) rot.push_back(fol[i]);             // a rotation row of its own
        else { fol2.push_back(fol[i]); fmeta2.push_back(fmeta[i]); }
    }
    fol.swap(fol2);
    fmeta.swap(fmeta2);
}

// The rows of one level: lv[0..R) are the rotation rows, tl.ext (from share_level) the extractions behind them.  Per row the
// lincomb descriptor, its terms, the look-up table, the latest tick that produces one of its inputs (row_need) and the
// noise bookkeeping; then the blocks: row outputs in row order, then per follower its output and its leader's body
// block if new.  keep_recs: a CaptureRec per row (while capturing), numbered rec_level.
int Engine::build_rows(const std::vector<Bid> &lv, size_t R, TickLevel &tl, std::vector<uint64_t> &row_need, bool keep_recs,
                       uint32_t rec_level) {
    if (!tl.ext.empty()) tl.body.assign(R, nullptr);
    row_need.assign(R, 0);
    for (size_t li = 0; li < R; li++) {
        const Bid b = lv[li];
        const BlockNode &n = nodes_[b];
        const BlockNode &s = nodes_[n.src];
        LinDesc d{};
        d.first_term = (uint32_t)tl.terms.size();
        // noise bookkeeping: the variance of the combination entering this bootstrap in units of one bootstrap output's
        // (uploads counted like outputs; extractions of one shared rotation as fully correlated: lin_c2)
        int64_t c2 = 0;
        uint64_t &need = row_need[li];
        if (s.kind == BlockNode::MAT) {
            tl.terms.push_back({s.dev, 1});
            d.n_terms = 1;
            need = std::max(need, s.ready_tick);
            c2 = s.var;
        } else if (s.kind == BlockNode::LIN) {
            for (const Term &t : s.terms) {
                const BlockNode &tb = nodes_[t.blk];
                if (tb.kind != BlockNode::MAT || !tb.dev)
                    return ctx.fail(-3, "internal: lincomb term not materialised at its level");
                tl.terms.push_back({tb.dev, t.coef});
                need = std::max(need, tb.ready_tick);
            }
            c2 = lin_c2(s.terms);
            d.n_terms = (uint32_t)s.terms.size();
            d.konst_body = (uint64_t)(s.konst & 31) << DELTA_LOG;
        } else {
            return ctx.fail(-3, "internal: PBS source is neither MAT nor LIN (node " + std::to_string(b) + " level " +
                                    std::to_string(n.level) + " lut " + std::to_string(n.lut) + ", source " +
                                    std::to_string(n.src) + " kind " + std::to_string((int)s.kind) + " level " +
                                    std::to_string(s.level) + " refs " + std::to_string(s.refs) + ")");
        }
        stats.max_input_sum_c2 = std::max<uint64_t>(stats.max_input_sum_c2, (uint64_t)c2);
        if (c2 > FHS_NOISE_BUDGET_SUM_C2 && std::getenv("FHS_DEBUG_C2")) {
            std::fprintf(stderr, "c2=%lld lut=%d terms:", (long long)c2, (int)n.lut);
            for (const Term &t : s.terms) std::fprintf(stderr, " %lld*b%u", (long long)t.coef, t.blk);
            std::fprintf(stderr, "\n");
        }
        tl.descs.push_back(d);
        tl.lut.push_back(n.lut);
        if (capture_max_rows && keep_recs)
            tl.recs.push_back(CaptureRec{rec_level, (uint32_t)li, n.lut, d.n_terms, c2, s.kind == BlockNode::LIN ? s.konst : 0,
                                         (uint32_t)R});
        uint64_t *o = alloc_block();
        if (!o) return ctx.fail(-2, "device block pool exhausted (hipMalloc failed)");
        tl.out.push_back(o);
    }
    for (ShareRow &f : tl.ext) {                         // a follower's own block; its leader also stores the body polynomial
        f.out = alloc_block();
        if (!f.out) return ctx.fail(-2, "device block pool exhausted (hipMalloc failed)");
        if (!tl.body[f.lead_row]) {
            tl.body[f.lead_row] = alloc_block();
            if (!tl.body[f.lead_row]) return ctx.fail(-2, "device block pool exhausted (hipMalloc failed)");
        }
    }
    return 0;
}

// The level's nodes become materialised (rotation rows lv[0..R) -> tl.out, followers -> tl.ext), the members of a shared
// rotation get its group number, and the inputs are released: later levels may recycle their blocks.  row_tick (the
// scheduled path): the tick that writes each rotation row; a follower is ready with its leader.
void Engine::commit_rows(const std::vector<Bid> &lv, const TickLevel &tl, const std::vector<uint64_t> *row_tick) {
    const size_t R = tl.out.size();
    std::vector<uint32_t> rot_of(tl.ext.empty() ? 0 : R, 0);
    for (const ShareRow &f : tl.ext)
        if (!rot_of[f.lead_row]) rot_of[f.lead_row] = ++rot_counter_ ? rot_counter_ : ++rot_counter_;
    for (size_t k = 0; k < lv.size(); k++) {
        BlockNode &n = nodes_[lv[k]];
        const size_t lead = k < R ? k : tl.ext[k - R].lead_row;
        const Bid src = n.src;
        n.kind = BlockNode::MAT;
        n.dev = k < R ? tl.out[k] : tl.ext[k - R].out;
        if (!tl.ext.empty()) n.rot = rot_of[lead];
        n.src = 0;
        n.level = 0;
        if (row_tick) n.ready_tick = (*row_tick)[lead];
        release(src);
    }
}

// ------------------------------------------------------------------------------------------
// level-skewed batching: jobs, ticks
// ------------------------------------------------------------------------------------------
int Engine::plan_job(bool run_now, bool first_level_only, bool stream_pump) {
    if (pending_.empty()) return 0;
    if (!run_now && level_parallel && ctx.dist.active())
        return ctx.fail(-3, "fhs_submit is not available in level-parallel mode");
    if (!planner && !ctx.key_loaded) return ctx.fail(-3, "server key not loaded");
    LevelMap by_level = collect_levels(first_level_only);
    uint64_t tick = next_tick_ - 1;                           // the job's first level goes to next_tick_ at the earliest
    const uint64_t job = ++job_counter_;
    std::vector<uint64_t> row_need;                           // per row: latest tick that produces one of its inputs
    for (auto lvit = by_level.begin(); lvit != by_level.end(); ++lvit) {
        std::vector<TickLevel> one(1);
        one[0].job = job;
        const size_t R = share_level(by_level, lvit, first_level_only, one[0].ext);
        if (int rc = build_rows(lvit->second, R, one[0], row_need, capture_live, 0)) return rc;   // (level: run_tick)
        if (run_now) {
            // nothing is scheduled (flush drained it): enqueue this level right away, then plan the next one meanwhile
            if (int rc = run_tick(one, level_parallel && ctx.dist.active())) return rc;
            commit_rows(lvit->second, one[0], nullptr);       // immediate recycling is safe: stream order
            continue;
        }
        auto nx = std::next(lvit);
        const size_t next_width = nx == by_level.end() ? 0 : nx->second.size();
        if (int rc = schedule_level(one[0], lvit->second, row_need, tick, stream_pump, next_width)) return rc;
    }
    return 0;
}

// ---- list scheduling at ROW granularity ----------------------------------------------------------------------------
// A row runs at the first tick after the one that produces its last input (and not before the tick after the
// previous level's, `tick`).  Rows of one level may therefore sit on different ticks: the rows that consume a result
// which was itself sent one tick later (round alignment below, or a dependent job) follow it, the others stay.
// row_need: in, per row the latest tick that produces one of its inputs; out, the row's own tick.
int Engine::schedule_level(TickLevel &tl, const std::vector<Bid> &lv, std::vector<uint64_t> &row_need, uint64_t &tick,
                           bool stream_pump, size_t next_width) {
    const size_t R = tl.descs.size();
    const uint64_t job = tl.job;
    const uint64_t t0 = tick + 1;
    uint64_t base = ~0ull, last = 0;
    for (size_t k = 0; k < R; k++) {
        row_need[k] = std::max(t0, row_need[k] + 1);      // now: the row's own tick
        base = std::min(base, row_need[k]);
        last = std::max(last, row_need[k]);
    }
    tick = base;
    // round alignment: with `cur` rows already scheduled for the base tick, keep only as many of this level's on-time
    // rows as fill whole rounds of the persistent kernel; the excess (less than one round) runs one tick later with
    // whatever is scheduled there -- only ITS consumers follow it, the rest of the next level does not wait
    size_t n_base = 0;
    for (size_t k = 0; k < R; k++) n_base += row_need[k] == base;
    if (balance_slots) {
        size_t cur = 0;
        auto it = sched_.find(base);
        if (it != sched_.end())
            for (const TickLevel &l : it->second) cur += l.descs.size();
        const size_t total = cur + n_base, rem = total % balance_slots;
        const size_t rounds = (total + balance_slots - 1) / balance_slots;
        size_t defer = 0;
        // only when the last round would be less than ~2/3 full overall: a group that already fills 95 % of its rounds
        // is left alone (the split costs its consumers one tick)
        // (jobs scheduled by hand share their ticks with jobs still to come: there only a level that is at least one
        // round wide by itself is split; a streaming flush knows the whole population of the tick)
        if ((stream_pump ? total : n_base) >= balance_slots && rem && rem < n_base &&
            total * 100 < rounds * balance_slots * 95)
            defer = rem;
        // a sliver in front of a wide level (what an automatic partial flush leaves of a level: 16 388 = 2 x 8192 + 4)
        // would pay one whole bootstrap alone: it joins the next tick, where the rows of the next level that do not
        // consume it run anyway
        if (stream_pump && !defer && total * 8 < balance_slots && next_width >= 2 * balance_slots) defer = n_base;
        for (size_t k = R; k-- > 0 && defer;)
            if (row_need[k] == base) { row_need[k] = base + 1; defer--; }
        for (size_t k = 0; k < R; k++) last = std::max(last, row_need[k]);
    }
    last_sched_tick_ = std::max(last_sched_tick_, last);  // before the releases of commit_rows
    commit_rows(lv, tl, &row_need);
    // hand the rows to their ticks (ascending): one TickLevel per job and tick, rows of several levels merged
    std::vector<uint64_t> ticks(row_need.begin(), row_need.begin() + R);
    std::sort(ticks.begin(), ticks.end());
    ticks.erase(std::unique(ticks.begin(), ticks.end()), ticks.end());
    for (uint64_t tk : ticks) {
        std::vector<TickLevel> &slot = sched_[tk];
        TickLevel *dst = nullptr;
        for (TickLevel &l : slot)
            if (l.job == job) dst = &l;
        if (!dst) {
            slot.emplace_back();
            dst = &slot.back();
            dst->job = job;
        }
        if (ticks.size() == 1 && dst->descs.empty()) {    // the common case: the whole level on one tick
            *dst = std::move(tl);
            break;
        }
        std::vector<uint32_t> moved(tl.ext.empty() ? 0 : R, 0);   // leader row -> its position in dst
        for (size_t k = 0; k < R; k++) {
            if (row_need[k] != tk) continue;
            LinDesc d = tl.descs[k];
            const uint32_t f = d.first_term;
            d.first_term = (uint32_t)dst->terms.size();
            dst->terms.insert(dst->terms.end(), tl.terms.begin() + f, tl.terms.begin() + f + d.n_terms);
            if (!tl.ext.empty()) {
                moved[k] = (uint32_t)dst->descs.size();
                dst->body.resize(dst->descs.size(), nullptr);
                dst->body.push_back(tl.body[k]);
            }
            dst->descs.push_back(d);
            dst->lut.push_back(tl.lut[k]);
            dst->out.push_back(tl.out[k]);
            if (tl.recs.size() == tl.descs.size()) dst->recs.push_back(tl.recs[k]);
        }
        for (const ShareRow &f : tl.ext)                       // followers travel with their leader's tick
            if (row_need[f.lead_row] == tk) dst->ext.push_back({moved[f.lead_row], f.K, f.out});
    }
    // streaming flush: every tick up to `base` is complete now (later levels cannot reach back) -- enqueue them while
    // the host plans the next level
    if (stream_pump)
        while (!sched_.empty() && sched_.begin()->first <= base)
            if (int rc = pump(1)) return rc;
    return 0;
}

int Engine::pump(size_t n_ticks) {
    for (size_t it = 0; it < n_ticks && !sched_.empty(); it++) {
        auto first = sched_.begin();
        const uint64_t tick = first->first;
        std::vector<TickLevel> levels = std::move(first->second);
        sched_.erase(first);
        if (int rc = run_tick(levels)) return rc;
        next_tick_ = tick + 1;
        pool_.tick_enqueued(tick);
    }
    if (sched_.empty() && last_sched_tick_ >= next_tick_) next_tick_ = last_sched_tick_ + 1;
    return 0;
}

int Engine::upload_plan(void *d_dst, const void *src, size_t bytes) {
    Staging *st = nullptr;
    for (Staging &c : staging_)
        if (!c.busy || hipEventQuery(c.done.peek()) == hipSuccess) { c.busy = false; if (!st || c.buf.cap >= bytes) st = &c; }
    if (!st && staging_.size() < 8) { staging_.emplace_back(); st = &staging_.back(); }
    if (!st) {                                           // every buffer is in flight: wait for the oldest
        st = &staging_[0];
        if (hipEventSynchronize(st->done.peek()) != hipSuccess) return ctx.fail(-2, "staging wait failed");
        st->busy = false;
    }
    if (st->buf.cap < bytes && st->buf.reserve(bytes + bytes / 2) != hipSuccess)      // (at least 1 MB)
        return ctx.fail(-2, "hipHostMalloc (plan staging) failed");
    if (!st->done.get()) return ctx.fail(-2, "hipEventCreate failed");
    std::memcpy(st->buf.ptr, src, bytes);
    hipError_t e = hipMemcpyAsync(d_dst, st->buf.ptr, bytes, hipMemcpyHostToDevice, ctx.stream);
    if (e == hipSuccess) e = hipEventRecord(st->done.peek(), ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "plan upload");
    st->busy = true;
    return 0;
}

// ------------------------------------------------------------------------------------------
// launch groups: lincomb -> keyswitch -> blind rotation over the rows of one or more job levels
// ------------------------------------------------------------------------------------------
void Engine::note_level(size_t width) {
    stats.levels += 1;
    if (stats.level_widths.size() < (1u << 20)) stats.level_widths.push_back((uint32_t)width);
    stats.max_level_width = std::max<uint64_t>(stats.max_level_width, width);
}

// The device layout of a launch group, defined here only: [descs | terms | lut | out pointers (16-byte aligned)], and
// with rotation sharing behind them [body pointer per row | one ExtractDesc per follower].  first_term becomes relative
// to the group's terms.
Engine::GroupView Engine::pack_group(const TickLevel *levels, size_t n_levels, std::vector<uint8_t> &host) const {
    GroupView v;
    size_t n_terms = 0;
    for (size_t j = 0; j < n_levels; j++) {
        v.width += levels[j].descs.size();
        n_terms += levels[j].terms.size();
        v.n_ext += levels[j].ext.size();
    }
    v.off_terms = v.width * sizeof(LinDesc);
    v.off_lut = v.off_terms + n_terms * sizeof(LinTerm);
    v.off_out = (v.off_lut + v.width * 4 + 15) & ~(size_t)15;
    v.off_body = v.off_out + v.width * sizeof(uint64_t *);
    v.off_ext = v.off_body + (v.n_ext ? v.width * sizeof(uint64_t *) : 0);
    v.total = v.off_ext + v.n_ext * sizeof(ExtractDesc);
    host.assign(v.total, 0);
    LinDesc *hd = reinterpret_cast<LinDesc *>(host.data());
    LinTerm *ht = reinterpret_cast<LinTerm *>(host.data() + v.off_terms);
    uint32_t *hl = reinterpret_cast<uint32_t *>(host.data() + v.off_lut);
    uint64_t **ho = reinterpret_cast<uint64_t **>(host.data() + v.off_out);
    uint64_t **hb = reinterpret_cast<uint64_t **>(host.data() + v.off_body);
    ExtractDesc *hx = reinterpret_cast<ExtractDesc *>(host.data() + v.off_ext);
    size_t di = 0, ti = 0, xi = 0;
    for (size_t j = 0; j < n_levels; j++) {
        const TickLevel &l = levels[j];
        for (size_t k = 0; k < l.descs.size(); k++) {
            LinDesc d = l.descs[k];
            d.first_term += (uint32_t)ti;
            hd[di + k] = d;
            hl[di + k] = lut_slot(l.lut[k]);                  // (ensure_luts has run: upload_group)
            ho[di + k] = l.out[k];
            if (v.n_ext) hb[di + k] = k < l.body.size() ? l.body[k] : nullptr;
        }
        for (const ShareRow &f : l.ext) hx[xi++] = ExtractDesc{l.out[f.lead_row], l.body[f.lead_row], f.out, f.K, 0};
        if (!l.terms.empty()) std::memcpy(ht + ti, l.terms.data(), l.terms.size() * sizeof(LinTerm));
        di += l.descs.size();
        ti += l.terms.size();
    }
    return v;
}

// room for a group of `width` rows whose packed form takes `bytes`; a buffer that grows waits for the stream (queued
// launches read the old one)
hipError_t Engine::grow_synced(DevBuf &b, size_t want) {
    if (b.cap >= want) return hipSuccess;
    hipError_t e = hipStreamSynchronize(ctx.stream);
    return e == hipSuccess ? b.reserve(want) : e;
}
int Engine::ensure_group_buffers(size_t width, size_t bytes) {
    hipError_t e = grow_synced(tick_buf_, bytes);
    if (e == hipSuccess) e = grow_synced(batch_in_, width * BIG_CT * 8);
    if (e == hipSuccess) e = grow_synced(ctx.ks_buf, width * SMALL_CT * 8);
    return e == hipSuccess ? 0 : ctx.hip_fail(e, "tick buffers");
}

// packs the group, makes room and uploads it: stream-ordered after the previous group's kernels, which read the old
// contents; pinned staging, so the host goes on
int Engine::upload_group(const TickLevel *levels, size_t n_levels, GroupView &v) {
    if (int rc = ensure_luts(levels, n_levels)) return rc;
    std::vector<uint8_t> host;
    v = pack_group(levels, n_levels, host);
    if (int rc = ensure_group_buffers(v.width, v.total)) return rc;
    return upload_plan(tick_buf_.ptr, host.data(), v.total);
}

// debug only: a strided sample of rows [first, first + cnt) of level `l`, which lie in batch_in_ from row `batch_row`
// on, goes to the host (synchronous copies).  `level`: live captures number the levels as the statistics do, captures
// through an all-at-once plan by their position in that flush.
int Engine::sample_capture(const TickLevel &l, size_t first, size_t cnt, size_t batch_row, uint32_t level) {
    const size_t stride = (cnt + capture_max_rows - 1) / capture_max_rows;
    for (size_t i = 0; i < cnt; i += stride) {
        const size_t at = capture_rows.size();
        capture_rows.resize(at + BIG_CT);
        hipError_t e = hipMemcpyAsync(capture_rows.data() + at, batch_in_.as<uint64_t>() + (batch_row + i) * BIG_CT, BIG_CT * 8,
                                      hipMemcpyDeviceToHost, ctx.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx.stream);
        if (e != hipSuccess) return ctx.hip_fail(e, "capture download");
        CaptureRec r = l.recs[first + i];
        r.level = level;
        capture_recs.push_back(r);
    }
    return 0;
}

// Rows [lo, lo + cnt) of the uploaded group `v`: lincomb -> (capture sample) -> keyswitch -> blind rotation.
// dense_out: the results go to its rows 0..cnt (a slice for an exchange); null: to the rows' own blocks (and the
// accumulator bodies of rotation leaders to theirs).  levels / first_level: the group's levels for the capture
// sampler (n_levels 0: none).
int Engine::launch_rows(const GroupView &v, size_t lo, size_t cnt, uint64_t *dense_out, const TickLevel *levels,
                        size_t n_levels, size_t first_level) {
    const uint8_t *dp = tick_buf_.as<uint8_t>();
    const LinDesc *d_desc = reinterpret_cast<const LinDesc *>(dp);
    const LinTerm *d_terms = reinterpret_cast<const LinTerm *>(dp + v.off_terms);
    const uint32_t *d_lut = reinterpret_cast<const uint32_t *>(dp + v.off_lut);
    uint64_t *const *d_out = reinterpret_cast<uint64_t *const *>(dp + v.off_out);
    uint64_t *const *d_body = reinterpret_cast<uint64_t *const *>(dp + v.off_body);
    hipError_t e = launch_lincomb(d_desc + lo, d_terms, batch_in_.as<uint64_t>(), (int)cnt, ctx.stream);
    if (e != hipSuccess) return ctx.hip_fail(e, "lincomb launch");
    size_t row0 = 0;
    for (size_t j = 0; j < n_levels && capture_max_rows; j++) {
        const TickLevel &l = levels[j];
        const size_t w = l.descs.size(), a = std::max(lo, row0), b = std::min(lo + cnt, row0 + w);
        if (l.recs.size() == w && a < b)
            if (int rc = sample_capture(l, a - row0, b - a, a - lo, (uint32_t)(first_level + j))) return rc;
        row0 += w;
    }
    if (int rc = ctx.keyswitch(batch_in_.as<uint64_t>(), cnt, ctx.stream)) return rc;
    return ctx.blind_rotate(ctx.ks_buf.as<uint64_t>(), d_lut + lo, d_luts_.as<uint64_t>(), luts_clean_, dense_out, dense_out ? nullptr : d_out + lo, cnt,
                            ctx.stream, v.n_ext && !dense_out ? d_body + lo : nullptr);
}

// rows 0..width of d_all (a gathered level, row order) -> the rows' own blocks; d_out: their pointer table on the device
int Engine::scatter_rows(const uint64_t *d_all, uint64_t *const *d_out, size_t width) {
    hipError_t e = launch_scatter_blocks(d_all, d_out, (int)width, ctx.stream);
    return e == hipSuccess ? 0 : ctx.hip_fail(e, "scatter launch");
}

// what a planner context WOULD run in this launch group (engine.h "plan trace")
void Engine::trace_group(const std::vector<TickLevel> &levels, size_t width) {
    for (auto &l : levels) {
        for (size_t k = 0; k < l.descs.size(); k++) {
            const LinDesc &d = l.descs[k];
            trace_.insert(trace_.end(), {TR_ROW, (uint64_t)(uintptr_t)l.out[k], l.lut[k], d.konst_body >> DELTA_LOG, d.n_terms});
            for (uint32_t t = 0; t < d.n_terms; t++) {
                trace_.push_back((uint64_t)(uintptr_t)l.terms[d.first_term + t].src);
                trace_.push_back((uint64_t)l.terms[d.first_term + t].coef);
            }
        }
        for (const ShareRow &f : l.ext)
            trace_.insert(trace_.end(), {TR_EXT, (uint64_t)(uintptr_t)l.out[f.lead_row], (uint64_t)(uintptr_t)f.out, f.K});
    }
    trace_.push_back(TR_GROUP_END);
    trace_.push_back(width);
}

// One launch group over the union of the job levels scheduled for a tick.  sharded: level-parallel mode -- this rank
// runs slice [rank*cap, (rank+1)*cap) of the group into the exchange buffer, the slices are all-gathered on the stream
// and scattered into the nodes' blocks (all enqueued, no host wait with RCCL).
int Engine::run_tick(std::vector<TickLevel> &levels, bool sharded) {
    size_t width = 0, n_ext = 0;
    for (auto &l : levels) { width += l.descs.size(); n_ext += l.ext.size(); }
    if (width == 0) return 0;
    for (auto &l : levels) note_level(l.descs.size());        // the full width, whatever this rank's slice
    const size_t world = sharded ? (size_t)ctx.dist.world : 1, rank = sharded ? (size_t)ctx.dist.rank : 0;
    const size_t cap = (width + world - 1) / world;
    const size_t lo = std::min(width, rank * cap), hi = std::min(width, lo + cap), cnt = hi - lo;
    stats.pbs_executed += cnt;
    if (n_ext && sharded) return ctx.fail(-3, "internal: rotation sharing in a level-parallel launch group");
    stats.pbs_extracted += n_ext;
    if (stats.group_rows.size() < (1u << 20)) stats.group_rows.push_back((uint32_t)cnt);
    auto free_bodies = [&] {                                  // the accumulator bodies' blocks go back to the pool
        for (auto &l : levels)
            for (uint64_t *b : l.body)
                if (b) free_block(b);
    };
    if (planner) {
        if (trace_plan) trace_group(levels, width);
        // nothing runs, but the exchange of a level-parallel launch group is accounted for like Dist::all_gather does
        if (sharded) { ctx.dist.n_gathers++; ctx.dist.bytes_sent += cap * BIG_CT * 8; }
        free_bodies();
        return 0;
    }
    if (hipSetDevice(ctx.device) != hipSuccess) return ctx.fail(-2, "hipSetDevice failed");
    GroupView v;
    if (int rc = upload_group(levels.data(), levels.size(), v)) return rc;
    if (!sharded) {
        // while capturing live: the rows are the ones the production path bootstraps, shared rotations included
        if (int rc = launch_rows(v, 0, width, nullptr, levels.data(), levels.size(), stats.levels - levels.size())) return rc;
        if (n_ext) {
            // the followers: further sample extractions of their leaders' accumulators (stream order: whoever gets the
            // bodies' blocks next runs behind this kernel)
            hipError_t e = launch_extract_shift(reinterpret_cast<const ExtractDesc *>(tick_buf_.as<uint8_t>() + v.off_ext),
                                                (int)n_ext, ctx.stream);
            if (e != hipSuccess) return ctx.hip_fail(e, "extract launch");
            free_bodies();
        }
    } else {
        hipError_t e = grow_synced(ctx.xchg_send, cap * BIG_CT * 8);
        if (e == hipSuccess) e = grow_synced(ctx.xchg_recv, world * cap * BIG_CT * 8);
        if (e != hipSuccess) return ctx.hip_fail(e, "level exchange buffers");
        if (cnt)
            if (int rc = launch_rows(v, lo, cnt, ctx.xchg_send.as<uint64_t>(), nullptr, 0, 0)) return rc;
        if (int rc = ctx.dist.all_gather(ctx.xchg_send.ptr, ctx.xchg_recv.ptr, cap * BIG_CT * 8, ctx.stream, ctx.err)) return rc;
        if (int rc = scatter_rows(ctx.xchg_recv.as<uint64_t>(),
                                  reinterpret_cast<uint64_t *const *>(tick_buf_.as<uint8_t>() + v.off_out), width))
            return rc;
    }
    if (hipEvent_t done = last_group_done_.get()) (void)hipEventRecord(done, ctx.stream);
    return 0;
}

int Engine::gather_blocks(const Bid *local, size_t n, std::vector<Bid> &out) {
    out.clear();
    if (!ctx.dist.active()) return ctx.fail(-3, "no distributed transport (fhs_dist_init)");
    if (n == 0) return 0;
    const size_t world = (size_t)ctx.dist.world, row = (size_t)BIG_CT * 8;
    // The partial blocks must be in the stream before the exchange is enqueued -- nothing more: unsubmitted work is
    // submitted as a job and only the ticks that produce these blocks are pumped, so jobs of later requests that are
    // scheduled (level-skewed batching) stay scheduled.  Level-parallel mode and linear-combination blocks drain.
    int rc = 0;
    bool drain = level_parallel;
    if (!drain && !pending_.empty()) rc = submit();
    if (rc) return rc;
    uint64_t need = 0;
    for (size_t k = 0; k < n; k++) {
        const BlockNode &b = nodes_[local[k]];
        if (b.kind == BlockNode::LIN || b.kind == BlockNode::PBS) drain = true;
        else if (b.kind == BlockNode::MAT) need = std::max(need, b.ready_tick);
    }
    if (drain) rc = flush();
    else
        while (!rc && !sched_.empty() && sched_.begin()->first <= need) rc = pump(1);
    if (rc) return rc;
    // Extractions of ONE shared rotation are correlated (lin_c2); a gathered block comes back as a fresh node on every
    // rank, so that relation would be lost in the exchange.  The sharded operations never send two members of one group
    // (their partials are AND / OR results over different inputs); a caller-supplied set that does is refused rather than
    // under-charged.  The rank's OWN blocks keep their bookkeeping across the exchange (below).
    for (size_t k = 0; k < n; k++) {
        const BlockNode &a = nodes_[local[k]];
        if (a.kind != BlockNode::MAT || !a.rot) continue;
        for (size_t q = 0; q < k; q++)
            if (nodes_[local[q]].kind == BlockNode::MAT && nodes_[local[q]].rot == a.rot)
                return ctx.fail(-3, "all-gather of two extractions of one shared blind rotation: their noise correlation would "
                                    "be lost on the receivers (refresh one of them, or fhs_set_rotation_sharing(ctx, 0))");
    }
    auto keep_own = [&](std::vector<Bid> &got) {             // own slice: the figures this rank already tracks
        const size_t r0 = (size_t)ctx.dist.rank * n;
        for (size_t k = 0; k < n && r0 + k < got.size(); k++) {
            const BlockNode &a = nodes_[local[k]];
            if (a.kind != BlockNode::MAT) continue;
            nodes_[got[r0 + k]].var = std::max(nodes_[got[r0 + k]].var, a.var);
            nodes_[got[r0 + k]].rot = a.rot;
        }
    };
    if (planner) {
        // a planner context exchanges nothing: count the all-gather like Dist::all_gather does and hand back world * n
        // fresh single-output blocks, so that the combine DAG can be recorded and levelised (multi-GPU projections)
        ctx.dist.n_gathers++;
        ctx.dist.bytes_sent += n * row;
        for (size_t i = 0; i < world * n; i++) out.push_back(from_device(nullptr));
        keep_own(out);
        return 0;
    }
    if (hipSetDevice(ctx.device) != hipSuccess) return ctx.fail(-2, "hipSetDevice failed");
    hipError_t e = grow_synced(ctx.xchg_send, n * row);
    if (e == hipSuccess) e = grow_synced(ctx.xchg_recv, world * n * row);
    if (e != hipSuccess) return ctx.hip_fail(e, "exchange buffers");
    for (size_t k = 0; k < n; k++)
        if ((rc = copy_block_to_device(local[k], ctx.xchg_send.as<uint64_t>() + k * BIG_CT, false, false))) return rc;
    if ((rc = ctx.dist.all_gather(ctx.xchg_send.ptr, ctx.xchg_recv.ptr, n * row, ctx.stream, ctx.err))) return rc;
    out.reserve(world * n);
    for (size_t i = 0; i < world * n; i++) {
        Bid b = from_device(ctx.xchg_recv.as<uint64_t>() + i * BIG_CT);
        if (!b) {
            for (Bid x : out) release(x);
            out.clear();
            return ctx.fail(-2, "import of a gathered block failed");
        }
        out.push_back(b);
    }
    keep_own(out);
    return 0;
}

// ------------------------------------------------------------------------------------------
// the all-at-once plan (fhs_flush_plan / fhs_flush_level_exec / fhs_flush_level_commit, and captures that are not live)
// ------------------------------------------------------------------------------------------
// Plans every pending level with the builder of plan_job, but as whole DAG levels in level order: no rotation sharing,
// no tick scheduling, no round alignment.  The nodes get their output blocks here; the levels wait in planned_ for
// exec_level, which counts them in the statistics when they run.
int Engine::plan_flush() {
    planned_.clear();
    planned_max_width_ = 0;
    if (pending_.empty()) return 0;
    if (!planner) {
        if (!ctx.key_loaded) return ctx.fail(-3, "server key not loaded");
        if (hipSetDevice(ctx.device) != hipSuccess) return ctx.fail(-2, "hipSetDevice failed");
    }
    LevelMap by_level = collect_levels(false);
    std::vector<uint64_t> row_need;
    for (auto &kv : by_level) {
        planned_.emplace_back();
        if (int rc = build_rows(kv.second, kv.second.size(), planned_.back(), row_need, true, (uint32_t)planned_.size() - 1)) return rc;
        commit_rows(kv.second, planned_.back(), nullptr);
        planned_max_width_ = std::max(planned_max_width_, kv.second.size());
    }
    return 0;
}

// Runs rows [lo, hi) of planned level k.  dense_out == nullptr: results go straight to the nodes' blocks;
// otherwise they are written as rows 0..hi-lo of dense_out (distributed mode, before the all-gather).
int Engine::exec_level(size_t k, size_t lo, size_t hi, uint64_t *dense_out) {
    if (k >= planned_.size()) return ctx.fail(-1, "level index out of range");
    const TickLevel &l = planned_[k];
    if (lo > hi || hi > l.descs.size()) return ctx.fail(-1, "slice out of range");
    const size_t cnt = hi - lo;
    if (cnt == 0) return 0;
    if (!planner) {
        if (hipSetDevice(ctx.device) != hipSuccess) return ctx.fail(-2, "hipSetDevice failed");
        GroupView v;
        if (int rc = upload_group(&l, 1, v)) return rc;
        if (int rc = launch_rows(v, lo, cnt, dense_out, &l, 1, k)) return rc;
    }
    if (stats.group_rows.size() < (1u << 20)) stats.group_rows.push_back((uint32_t)cnt);
    stats.pbs_executed += cnt;
    if (lo == 0 || dense_out) note_level(l.descs.size());
    return 0;
}

// Distributed mode: rows 0..width of d_all (the gathered level, row order) -> the nodes' blocks.  Other work may have
// used the stream since exec_level: the level's pointer table is uploaded again.
int Engine::commit_level(size_t k, const uint64_t *d_all) {
    if (k >= planned_.size()) return ctx.fail(-1, "level index out of range");
    const TickLevel &l = planned_[k];
    if (!planner) {
        if (hipSetDevice(ctx.device) != hipSuccess) return ctx.fail(-2, "hipSetDevice failed");
        const size_t bytes = l.out.size() * sizeof(uint64_t *);
        if (int rc = ensure_group_buffers(0, bytes)) return rc;
        if (int rc = upload_plan(tick_buf_.ptr, l.out.data(), bytes)) return rc;
        if (int rc = scatter_rows(d_all, tick_buf_.as<uint64_t *>(), l.out.size())) return rc;
    }
    if (k + 1 == planned_.size()) planned_.clear();
    return 0;
}

}  // namespace fhs
