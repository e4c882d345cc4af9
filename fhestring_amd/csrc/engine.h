// Lazy DAG engine: records shortint-block operations, folds constants, levelises the pending
// programmable bootstraps and launches each dependency level as one wide batch.
//
// The reference evaluates every FheAsciiChar op eagerly and blocking; behind that
// API a GPU would only ever see 4-8 PBS at a time.  Here an op only creates nodes.  The pending
// bootstraps are planned LEVEL BY LEVEL (plan_job): rows that differ only in a trivial constant
// share one blind rotation, the level's rows are uploaded and enqueued as one launch group
// (lincomb -> keyswitch -> blind rotation, run_tick) while the host plans the next level -- or, for
// submitted jobs and round alignment, scheduled on ticks whose launch groups merge the levels of
// several jobs.  A level that is already wide is peeled and run while the DAG is still being
// recorded.  One level builder and one launch-group path serve all of it, the all-at-once plan of
// fhs_flush_plan / fhs_flush_level_exec / fhs_flush_level_commit included.
#pragma once
#include <cstdint>
#include <map>
#include <unordered_map>
#include <utility>
#include <vector>

#include "context.h"
#include "engine_resources.h"
#include "luts.h"
#include "select_kernels.h"

namespace fhs {

using Bid = uint32_t;   // block id; 0 is never valid

struct Term {
    int64_t coef;
    Bid blk;
};

struct BlockNode {
    enum Kind : uint8_t { FREE, TRIV, MAT, LIN, PBS };
    Kind kind = FREE;
    uint8_t triv = 0;        // TRIV: value mod 32
    uint16_t lut = 0;        // PBS
    uint16_t var = 1;        // MAT: noise variance in units of one bootstrap output's (1 = a bootstrap output or a fresh
                             // upload; more for a linear combination that was materialised for a download / an export,
                             // or an upload declared noisier with fhs_char_set_noise)
    int32_t konst = 0;       // LIN: constant (mod 32)
    uint32_t level = 0;      // PBS depth since the last flush
    uint32_t refs = 0;
    uint32_t gen = 0;        // bumped every time the slot is handed out again (common-subexpression table keys)
    uint64_t nk = 0;         // PBS (fused mode): hash of (table, terms) WITHOUT the trivial constant -- rows with equal nk will
                             // share a blind rotation (plan_job); 0 = counts as a rotation of its own
    uint32_t rot = 0;        // MAT: rotation group (non-zero for the leader and the followers of ONE shared blind rotation):
                             // their noises are correlated, the bookkeeping adds their coefficients before squaring
    uint8_t packs = 0;       // MAT: ring packings inside this block's noise (a block restored from the string store: the entry's
                             // cycle count; a materialised sum: the maximum over its terms; 0 for everything else, every
                             // bootstrap output included).  True variance <= var * (1 + packs * 2^-11.6).
    uint64_t ready_tick = 0; // MAT produced by a scheduled (not yet enqueued) job level: the tick that writes it
    Bid src = 0;             // PBS: input block
    uint64_t *dev = nullptr; // MAT: device ciphertext (2049 u64)
    std::vector<Term> terms; // LIN
};

struct EngineStats {
    uint64_t pbs_executed = 0, pbs_folded = 0, levels = 0, max_level_width = 0;
    uint64_t pbs_shared = 0;         // bootstraps not run because an identical one (same input combination, same LUT) exists
    uint64_t max_input_sum_c2 = 0;   // largest sum of squared coefficients of any executed bootstrap's input
    std::vector<uint32_t> level_widths;   // width of every dependency level executed since the last reset (capped)
    uint64_t pbs_extracted = 0;      // results obtained as a further sample extraction of a shared blind rotation (not in pbs_executed)
    std::vector<uint32_t> group_rows;     // rows THIS rank ran in every launch group (lincomb -> keyswitch -> blind rotation) since the last reset (capped)
};

class Engine {
  public:
    Context ctx;
    EngineStats stats;
    int mode = 0;   // 0 as written, 1 fused (string layer)
    // Planner context (fhs_ctx_create_planner): records DAGs, levelises them and keeps the statistics (PBS count, level
    // widths, noise bookkeeping) but owns no device and executes nothing; downloads fail.  Host logic only.
    bool planner = false;

    int on_key_loaded();
    // a real context waits for its stream (nothing queued may read what the members are about to free); a planner makes
    // no HIP call
    ~Engine();

    // ---- block graph (all returned ids carry one reference owned by the caller) ----
    Bid triv(int v);
    Bid from_host(const uint64_t *ct);          // uploads 2049 words
    // `count` ciphertexts of 2049 words each, back to back on the host: one copy through a pinned staging buffer and one
    // scatter launch into the pool blocks instead of one pageable copy (~10 us) per block
    int from_host_many(const uint64_t *cts, size_t count, Bid *out);
    // The seeded twin (fhs_upload_string_compressed): `count` blocks of a compressed string, global block indices
    // first_block .. first_block + count - 1, bodies[count].  Only body and destination pointer cross the bus; the
    // masks are regenerated from the seed straight into the pool blocks (seeded_kernels.hip).
    int from_compressed_many(const uint32_t seed[8], const uint64_t *bodies, size_t count, uint64_t first_block, Bid *out);
    // The public-key twin (fhs_upload_string_public): `count` blocks of a compact string, global block indices
    // first_block .. first_block + count - 1; mask32 / body32 are the WHOLE string's.  The u32 masks of the groups a
    // pass touches, its u32 bodies and the destination pointers cross the bus; every block is a sample extraction
    // written straight into its pool block (pk_kernels.hip).
    int from_public_many(const uint32_t *mask32, const uint32_t *body32, size_t count, uint64_t first_block, Bid *out);
    Bid from_device(const uint64_t *d_ct);      // D2D copy
    Bid lin(const Term *terms, size_t n, int konst);
    Bid pbs(Bid x, int lut);
    void retain(Bid b);
    void release(Bid b);
    const BlockNode &node(Bid b) const { return nodes_[b]; }
    bool is_triv(Bid b) const { return nodes_[b].kind == BlockNode::TRIV; }
    int triv_val(Bid b) const { return nodes_[b].triv; }
    // sum of squared coefficients of a block as a combination of bootstrap outputs / uploads (its noise variance in
    // units of one bootstrap output's): 0 trivial, 1 materialised or pending bootstrap, sum c^2 for a linear combination
    int64_t sum_c2(Bid b) const;
    // ... of a flattened combination.  The leader and the followers of one shared blind rotation are extractions of one
    // accumulator: their errors are correlated (measured: rho falls linearly with the constant difference from +0.45 to
    // -0.45, profiles/r05_rotation_sharing_rho.txt), so a group contributes sum c^2 + 1/2 ((sum |c|)^2 - sum c^2)
    int64_t lin_c2(const std::vector<Term> &terms) const;
    int64_t term_var(Bid b) const { return nodes_[b].kind == BlockNode::MAT ? nodes_[b].var : 1; }   // of a flattened term
    int set_var(Bid b, uint64_t v, bool check_only = false);                         // MAT blocks only (fhs_char_set_noise)

    int flush();
    // ---- level-skewed batching of independent jobs (fhs_submit / fhs_pump) ----------------------------------------
    // submit() plans the pending PBS as a JOB and schedules its dependency levels on consecutive TICKS starting at the
    // next one (later if an input is produced by an earlier job that has not run yet); pump(n) enqueues the next n ticks,
    // each as ONE launch group (lincomb -> keyswitch -> blind rotation) over the union of every job's level scheduled for
    // it.  With one submit + one pump per request the narrow tail levels of request k ride in the wide launch of
    // request k + 1 instead of paying one bootstrap latency each on an almost empty GPU.  flush() drains all ticks.
    // Automatic partial flush: once this many pending bootstraps have all their inputs available (depth 1), THAT level is
    // planned and enqueued while the caller keeps building the rest of the DAG; deeper nodes stay pending (their depth
    // drops by one), so the narrow later levels still merge across the whole operation.  A 1024-character replace records
    // 256 k bootstraps in ~0.25 s of host time: without this the GPU idles through all of it, and with 8 GPUs that is as
    // long as the computation.  0 = off.  Not used while jobs are scheduled by hand (submit / pump) or inputs are captured.
    size_t auto_flush_pending = 8192;
    // fhs_submit scheduling: a job level that would leave the launch group of its tick with a partly filled last round
    // of the persistent blind-rotation kernel (width not a multiple of the resident workgroup slots) sends the excess
    // rows to the next tick instead (their consumers move with them).  0 = off.
    size_t balance_slots = 0;
    int submit() { manual_jobs_ = true; return plan_job(false); }
    int pump(size_t n_ticks);
    bool has_scheduled() const { return !sched_.empty(); }
    // Level-parallel execution INSIDE the library (fhs_dist_level_parallel): every rank holds the same ciphertexts and
    // records the same DAG; flush() then runs slice [rank*cap, (rank+1)*cap) of every level, all-gathers the slices on
    // the context's stream (ctx.dist: RCCL, no host wait between levels) and installs the gathered level.
    bool level_parallel = false;
    // Rotation sharing (fused mode): rows of one level that differ only in the trivial constant of their input share one
    // keyswitch + blind rotation (plan_job).  fhs_set_rotation_sharing(ctx, 0) switches it off (A/B measurements, tests).
    bool share_rotations = true;
    // Gathers `n` blocks per rank: local[k] of every rank -> out[r * n + k] (fresh MAT blocks owned by the caller).
    // Flushes the local DAG first; everything is enqueued on the context's stream.
    int gather_blocks(const Bid *local, size_t n, std::vector<Bid> &out);
    // distributed execution (one process per GPU, identical DAGs on every rank): plan once, then per
    // level every rank runs its slice into a dense buffer, the caller all-gathers, commit scatters.
    // plan_flush is plan_job's level builder without rotation sharing and without scheduling: whole DAG levels in
    // level order, kept until exec_level runs them through the launch-group path of run_tick.
    int dist_rank = 0, dist_world = 1;
    int plan_flush();
    size_t planned_levels() const { return planned_.size(); }
    size_t level_width(size_t k) const { return planned_[k].descs.size(); }
    size_t planned_max_width() const { return planned_max_width_; }
    int exec_level(size_t k, size_t lo, size_t hi, uint64_t *dense_out);
    int commit_level(size_t k, const uint64_t *d_all);
    int read_block(Bid b, uint64_t *host_out);        // flushes if needed
    // diagnostic (fhs_debug_read_lut): the device copy of a table's polynomial [2048]; a user table that this context has
    // not used yet is expanded first
    int read_lut(int lut_id, uint64_t *host_out);
    // `count` blocks into consecutive 2049-word rows on the host: one gather launch and one copy through the pinned staging
    // buffer per 2048 blocks instead of one synchronous copy per block (the twin of from_host_many)
    int read_many(const Bid *b, size_t count, uint64_t *host_out);
    // packed download (pack_kernels.hip): ring-packs the blocks in groups of 2048 and stores them at 16 bits; mask16
    // [groups][2048], body16 [count].  mask64 / body64 (diagnostic, may be null): the 64-bit GLWEs [groups][2048].
    // recipient: the 16-bit words leave under the client key the context's re-key key leads to (rekey_packed_kernel in
    // place of the storage switch, one launch per pass); mask64 / body64 stay the tree's output under the sender's key.
    int read_packed(const Bid *b, size_t count, uint16_t *mask16, uint16_t *body16, uint64_t *mask64, uint64_t *body64,
                    bool recipient = false);
    // ---- device-resident string store (store_kernels.hip; include/fhestring_hip.h, "device-resident string store") ----
    // An entry is one block sequence parked in the compact-string format: mask32[ceil(n / 2048)][2048] | body32[n] in ONE
    // device allocation of its exact size, plus what the bookkeeping knew about every block at store_put (host side).
    struct StoreEntry {
        size_t n_blocks = 0;
        DevBuf buf;                       // empty on a planner context
        std::vector<uint16_t> var;        // BlockNode::var (1 for a trivial block: it comes back as an ordinary ciphertext)
        std::vector<uint8_t> cycles;      // packings inside the block's noise, this entry's included (0: imported fresh)
        std::vector<uint32_t> rot;        // BlockNode::rot, the engine's id verbatim
        uint8_t rekeys = 0;               // re-keys inside the entry's noise (store_rekey); not exported, 0 after an import
        size_t groups() const { return (n_blocks + 2047) / 2048; }
        size_t bytes() const { return groups() * 2048 * 4 + n_blocks * 4; }
    };
    static constexpr int STORE_MAX_CYCLES = 16;   // FHS_STORE_MAX_CYCLES
    // Parks `count` blocks (any block read_packed takes; pending work is flushed, sums are materialised) through the packing
    // tree and the 32-bit switch, all on the device.  A planner context records the metadata only.
    int store_put(const Bid *b, size_t count, uint64_t *id_out);
    // Blocks [first, first + count) of an entry as fresh MAT blocks with the entry's var / rot / cycles restored: passes of
    // up to 4096 blocks, only the destination pointer table crosses the bus.  Needs no key.
    int store_get(uint64_t id, size_t first, size_t count, Bid *out);
    int store_drop(uint64_t id);
    const StoreEntry *store_entry(uint64_t id) const;
    void store_stats(size_t *entries, size_t *blocks, size_t *bytes) const;
    // meta[t]: bits 0-15 var, 16-23 cycles, 32-63 the rotation group renumbered 1..k within the entry (0 = none)
    int store_export(uint64_t id, uint32_t *mask32, uint32_t *body32, uint64_t *meta);
    // one H2D copy, no kernel; meta == nullptr: every block a fresh upload (var 1, no group, no packing)
    int store_import(const uint32_t *mask32, const uint32_t *body32, const uint64_t *meta, size_t n_blocks, uint64_t *id_out);
    // Re-keys an entry to another client key with the context's re-key key (rekey_kernels.hip): in place (id_out ==
    // nullptr), or into a new entry that inherits var / cycles / rot and rekeys + 1.  A planner does the bookkeeping only.
    static constexpr int STORE_MAX_REKEYS = 255;   // FHS_STORE_MAX_REKEYS
    bool planner_rekey_key = false;                // planner only: fhs_load_rekey_key was given a key (nothing is converted)
    int store_rekey(uint64_t id, uint64_t *id_out);
    // Characters [first_char, first_char + count) of an entry in the windowed packed form, under the
    // entry's key or, recipient, under the key the context's re-key key leads to: mask16[covering groups][2048],
    // body16[4 count].  One launch on the context's stream (store_switch16_kernel / rekey_entry_packed_kernel), two copies,
    // one sync; no pool block, no node, no packing key, and the entry stays as it is.
    int store_read_packed(uint64_t id, size_t first_char, size_t count, bool recipient, uint16_t *mask16, uint16_t *body16);
    // Fetches one row of entry `id`, read as rows of row_chars characters, by the encrypted index in `query` (`bits` GGSWs,
    // fhs_client_select_query) into a NEW entry of row_chars characters (select_kernels.hip): one
    // launch per tree level and per rotate bit on the context's stream, no bootstrap, no pool block, no key.  The result's
    // blocks take the maxima of figure and cycles over the rows, one fresh rotation group if any candidate has one, and
    // rekeys + SELECT_REKEY_COST per launch.  A planner does the bookkeeping only.
    // q holds n queries of one form: n new entries with consecutive ids in ids_out[n], each with
    // bookkeeping of its own, from one conversion launch and one CMux launch per level and bit.  Atomic: an error creates
    // nothing.  batch: the call is fhs_store_select_batch, whose workspace is limited (FHS_SELECT_BATCH_MAX_BYTES).
    struct SelectQueries {
        int form;                        // FHS_SELECT_FORM_*
        const uint32_t *seeds;           // SEEDED: [n][8]
        const uint64_t *const *queries;  // n pointers: full words, or bodies
        size_t n;
    };
    int store_select(uint64_t id, size_t row_chars, const SelectQueries &q, int bits, bool batch, uint64_t *ids_out);
    // converted queries plus both level buffers of n queries, bytes; 0 for a refused shape or n
    static size_t select_batch_bytes(size_t n_chars, size_t row_chars, size_t n);
    // diagnostic: the same launches on host words, the arguments of fhs_store_select_host (one query)
    int debug_select(const SelectQueries &q, int bits, const uint32_t *mask32, const uint32_t *body32, size_t n_blocks,
                     size_t row_chars, uint32_t *mask_out, uint32_t *body_out);
    // diagnostic: the conversion kernel alone on one query
    int debug_select_query(const SelectQueries &q, int bits, double *out);
    // diagnostic: the kernel on host words of any block count; the outputs may be the inputs
    int debug_rekey(const uint32_t *mask32, const uint32_t *body32, size_t n_blocks, uint32_t *mask_out, uint32_t *body_out);
    // diagnostic: the recipient download's kernel alone on host words, mask64 / body64 [ceil(n_blocks / 2048)][2048]
    int debug_rekey_packed(const uint64_t *mask64, const uint64_t *body64, size_t n_blocks, uint16_t *mask16, uint16_t *body16);
    // flushes if needed (do_flush = false: the caller has made sure the block's tick is enqueued); wait=false: enqueue only
    int copy_block_to_device(Bid b, uint64_t *d_out, bool wait = true, bool do_flush = true);
    uint64_t blocks_live() const { return pool_.live(); }
    // ---- block pool: accounting and trimming ----
    void pool_stats(uint64_t out[6]) const { pool_.stats(out); }
    // Flushes, then gives back the chunks the pool does not need for its live blocks and `keep_free_blocks` more
    // (BlockPool::plan_trim).  compact: the live blocks of the victims first move into free slots of the kept chunks
    // (pool_move_blocks_kernel, passes of up to POOL_MOVE_MAX_BATCH blocks, only the pointer tables cross the bus) and
    // their nodes get the new address; otherwise only victims that hold no live block go.  A planner only flushes.
    static constexpr size_t POOL_MOVE_MAX_BATCH = 2048;   // blocks per launch: one chunk's worth, 33.6 MB
    int pool_trim(bool compact, size_t keep_free_blocks, uint64_t *blocks_moved, uint64_t *bytes_released);

    // ---- debug: capture of PBS inputs (the linear-combination results entering keyswitch) ----
    // Noise-margin tests download a sample of every level's inputs and measure their phase error with the client
    // key; nothing here sees a secret.  capture_max_rows == 0: off.
    struct CaptureRec { uint32_t level, index, lut, n_terms; int64_t sum_c2; int32_t konst; uint32_t width; };
    size_t capture_max_rows = 0;
    // capture_live: sample inside the ordinary execution path (plan_job / run_tick: rotation sharing, round alignment and
    // tick scheduling as in production; records numbered like stats.levels, width = the level's rotation rows) instead of
    // the all-at-once plan of plan_flush (unshared, whole levels; records numbered by their level within the flush)
    bool capture_live = false;
    std::vector<uint64_t> capture_rows;      // [n][2049]
    std::vector<CaptureRec> capture_recs;

    // ---- debug: plan trace (planner contexts; tests and bench.py's CPU-baseline leg) ----
    // While on, a planner context writes what it WOULD run as a flat list of 64-bit words (block tokens are the planner's
    // unique fake pointers): uploads in order, every launch group row by row (output token, LUT id, constant, terms), the
    // shared extractions, a group end.  A host executor replays it with any PBS implementation -- the CPU oracle runs the
    // product's fused DAGs that way (the checker's plan_exec.py); nothing in the product reads it back.
    enum : uint64_t { TR_UPLOAD = 1, TR_ROW = 2, TR_EXT = 3, TR_GROUP_END = 4 };
    bool trace_plan = false;
    std::vector<uint64_t> trace_;
    // [kind 0 TRIV / 1 MAT / 2 LIN / 3 pending, value or constant, n_terms, (token, coef)...] of one block
    void describe_block(Bid b, std::vector<uint64_t> &out) const;

    // ---- char handles (fhs_char_t) ----
    struct CharRec { Bid b[4]; bool used; };
    uint64_t new_char(const Bid b[4]);   // takes over the 4 references
    bool valid_char(uint64_t h) const { return h >= 1 && h <= chars_.size() && chars_[h - 1].used; }
    const Bid *char_blocks(uint64_t h) const { return chars_[h - 1].b; }
    void free_char(uint64_t h);

  private:
    std::vector<BlockNode> nodes_{1};   // slot 0 reserved
    std::vector<Bid> free_nodes_;
    struct Pend { Bid id; uint32_t gen; };                    // gen: a released pending node's slot may be reused before
    std::vector<Pend> pending_;                               // the flush; the stale entry must not stand for the new node
    std::vector<CharRec> chars_;
    std::vector<uint64_t> free_chars_;

    BlockPool pool_{planner};
    uint64_t *alloc_block() { return pool_.alloc(); }
    void free_block(uint64_t *p) { pool_.free(p, last_sched_tick_, next_tick_); }
    // whole-string uploads (from_host_many / from_compressed_many / from_public_many) and store_get
    TransferBuffer xfer_;
    int undo_upload(Bid *out, size_t count);                   // releases what was made, zeroes out[], returns -1
    Bid copy_in(const uint64_t *src, hipMemcpyKind kind);
    bool new_mat_blocks(size_t n, Bid *out, uint64_t *ptrs);
    int plan_upload(size_t count, Bid *out);
    bool send_pass(size_t n, Bid *out, size_t ptr_at, size_t at, size_t words);

    // LUT polynomials on the device: the catalogue, then the user tables THIS context has used, in order of first use
    // (DESIGN.md section 21).  The array grows only behind a drained stream (ensure_luts): a queued launch group reads
    // the address it was launched with; a scheduled one (sched_, planned_) holds table ids and gets its slots and the
    // array's address when it is uploaded.
    DevBuf d_luts_;
    // every word of the array has its low 8 bits clear (Context::blind_rotate's luts_clean): taken over the catalogue when it
    // is uploaded; a user table is 16 values << 59 and their negations (expand_user_luts_kernel) and cannot change it
    bool luts_clean_ = false;
    size_t lut_slots_ = LUT_COUNT, lut_cap_ = LUT_COUNT;      // polynomials written / room
    std::unordered_map<uint32_t, uint32_t> lut_slot_;         // user table id -> its slot
    uint32_t lut_slot(uint32_t id) const { return id < LUT_COUNT ? id : lut_slot_.at(id); }
    int ensure_luts(const uint32_t *ids, size_t n);           // expands the user tables among ids[n] that are not resident
    DevBuf plan_buf_, batch_in_;

    // rotation sharing (plan_job): a follower row is a further sample extraction of its leader's blind rotation
    struct ShareRow {
        uint32_t lead_row;                // position of the leader among the rotation rows of the same TickLevel
        uint32_t K;                       // negacyclic coefficient to extract: 128 x (constant difference mod 32)
        uint64_t *out;                    // the follower's own block
    };
    struct TickLevel {
        std::vector<LinDesc> descs;       // first_term relative to `terms`
        std::vector<LinTerm> terms;
        std::vector<uint32_t> lut;
        std::vector<uint64_t *> out;
        std::vector<uint64_t *> body;     // empty, or per rotation row: where the accumulator's body polynomial goes (leaders)
        std::vector<ShareRow> ext;        // followers of this level's leaders
        std::vector<CaptureRec> recs;     // per row, only while capturing
        uint64_t job = 0;                 // rows of one job that land on the same tick share one TickLevel
    };
    int ensure_luts(const TickLevel *levels, size_t n_levels);
    std::vector<TickLevel> planned_;      // plan_flush: whole levels waiting for exec_level / commit_level
    size_t planned_max_width_ = 0;
    std::map<uint64_t, std::vector<TickLevel>> sched_;            // tick -> job levels to run in that launch group
    uint64_t next_tick_ = 1, last_sched_tick_ = 0;
    bool manual_jobs_ = false;           // the caller schedules jobs itself (fhs_submit): no automatic partial flushes
    bool in_auto_flush_ = false;
    int auto_flush_rc_ = 0;              // first error of an automatic partial flush, reported by the next flush()
    std::string auto_flush_err_;
    DevBuf tick_buf_;
    // ---- one launch group (engine.cpp): byte offsets of its packed form in tick_buf_ ----
    struct GroupView { size_t width = 0, n_ext = 0, off_terms = 0, off_lut = 0, off_out = 0, off_body = 0, off_ext = 0, total = 0; };
    GroupView pack_group(const TickLevel *levels, size_t n_levels, std::vector<uint8_t> &host) const;
    hipError_t grow_synced(DevBuf &b, size_t want);      // a buffer that grows waits for the stream first
    int ensure_group_buffers(size_t width, size_t bytes);
    int upload_group(const TickLevel *levels, size_t n_levels, GroupView &v);
    int launch_rows(const GroupView &v, size_t lo, size_t cnt, uint64_t *dense_out, const TickLevel *levels, size_t n_levels,
                    size_t first_level);
    int sample_capture(const TickLevel &l, size_t first, size_t cnt, size_t batch_row, uint32_t level);
    int scatter_rows(const uint64_t *d_all, uint64_t *const *d_out, size_t width);
    void note_level(size_t width);
    void trace_group(const std::vector<TickLevel> &levels, size_t width);
    // sharded: level-parallel mode -- this rank runs slice [rank*cap, (rank+1)*cap) of the group into the exchange buffer,
    // the slices are all-gathered on the stream and scattered into the nodes' blocks
    int run_tick(std::vector<TickLevel> &levels, bool sharded = false);
    // ---- the level builder (plan_job and plan_flush) ----
    using LevelMap = std::map<uint32_t, std::vector<Bid>>;
    void reset_depth1();
    LevelMap collect_levels(bool first_level_only);
    size_t share_level(LevelMap &by_level, LevelMap::iterator lvit, bool first_level_only, std::vector<ShareRow> &followers);
    void unshare_over_budget(const LevelMap &by_level, LevelMap::const_iterator lvit, bool first_level_only,
                             std::vector<Bid> &rot, std::vector<Bid> &fol, std::vector<ShareRow> &fmeta);
    int build_rows(const std::vector<Bid> &lv, size_t R, TickLevel &tl, std::vector<uint64_t> &row_need, bool keep_recs,
                   uint32_t rec_level);
    void commit_rows(const std::vector<Bid> &lv, const TickLevel &tl, const std::vector<uint64_t> *row_tick);
    int schedule_level(TickLevel &tl, const std::vector<Bid> &lv, std::vector<uint64_t> &row_need, uint64_t &tick,
                       bool stream_pump, size_t next_width);
    // plans the pending PBS level by level; run_now: every level is enqueued as soon as it is planned (the host plans level
    // k + 1 while the GPU runs level k), otherwise the levels are scheduled on ticks (submit)
    // stream_pump (scheduled path only): enqueue every tick as soon as no later level can add rows to it
    int plan_job(bool run_now, bool first_level_only = false, bool stream_pump = false);
    uint64_t job_counter_ = 0;
    uint32_t rot_counter_ = 0;           // rotation groups handed out (BlockNode::rot)
    size_t n_depth1_ = 0;                // pending bootstraps whose inputs are all available
    // ... and how many blind ROTATIONS they are once rows that differ only in a trivial constant share one: what the
    // automatic partial flush counts in (a round of the persistent kernel is 1024 rotations, not 1024 results)
    std::unordered_map<uint64_t, uint32_t> depth1_keys_;
    size_t n_depth1_solo_ = 0;           // depth-1 nodes without a share key
    size_t depth1_rotations() const { return n_depth1_solo_ + depth1_keys_.size(); }
    void depth1_add(const BlockNode &n) { if (n.nk) depth1_keys_[n.nk]++; else n_depth1_solo_++; }
    size_t peel_limit_ = 0;              // automatic partial flush of an idle GPU: take this many ready rows (0 = all)
    Event last_group_done_{hipEventDisableTiming};   // recorded behind every launch group: tells whether the GPU has run dry
    uint32_t idle_poll_ = 0;
    // Pinned staging for plan uploads: a hipMemcpyAsync from PAGEABLE memory blocks the host until the stream reaches
    // the copy, i.e. until the previous launch group has finished -- the host could never plan ahead of the GPU.  A small
    // ring of pinned buffers, each guarded by an event recorded after its copy, keeps the upload asynchronous.
    struct Staging { PinnedBuf buf; Event done{hipEventDisableTiming}; bool busy = false; };
    std::vector<Staging> staging_;
    int upload_plan(void *d_dst, const void *src, size_t bytes);

    // Common-subexpression table of the fused string layer: (LUT, constant, [(block, generation, coefficient)...]) ->
    // the bootstrap node that already computes it.  Nodes are immutable, so an entry stays valid while its node lives.
    // Keys are 128-bit order-independent hashes of the terms (two independent 64-bit mixes: a false match needs both to
    // collide, ~2^-128 per pair), so a lookup allocates nothing.
    struct CseEntry { uint64_t h2; Bid id; uint32_t gen; };
    std::unordered_map<uint64_t, CseEntry> cse_;

    Bid new_node();
    int materialize_lin(Bid b);
    // What read_packed and store_put share: flush, sums become blocks; then per pass of up to four groups the leaf table
    // and the 11 tree levels, which leave the pass's GLWEs [groups][2][2048] in ctx.pack_ws[0].
    int prepare_packing(const Bid *b, size_t count);
    // one re-key launch over the groups of n_blocks blocks (device pointers, entry layout; out may be in), on the stream
    hipError_t rekey_words(const uint32_t *d_mask, const uint32_t *d_body, uint32_t *d_mask_out, uint32_t *d_body_out,
                           size_t n_blocks);
    // one launch of the recipient download's kernel: level-11 GLWEs [groups][2][2048] -> 16-bit words under the new key
    hipError_t rekey_packed_words(const uint64_t *d_glwe, uint16_t *d_mask16, uint16_t *d_body16, size_t n_blocks);
    // the select's launches from device words of the entry layout, all queries of q per launch
    // dst[y] (host array of device pointers): mask[2048] | body[4 row_chars] of query y's result
    hipError_t select_words(const SelectQueries &q, const uint32_t *d_mask, const uint32_t *d_body, size_t n_blocks,
                            const SelectShape &sh, uint32_t *const *dst);
    // upload and conversion into ctx.sel_query; dst (may be null) travels along, *d_table is its place on the device
    hipError_t select_queries_to_ntt(const SelectQueries &q, int bits, uint32_t *const *dst, uint32_t *const **d_table);
    hipError_t pack_tree_pass(const Bid *b, size_t n, size_t groups);
    std::map<uint64_t, StoreEntry> store_;
    uint64_t store_ids_ = 0;             // ids handed out: never reused inside a context
};

// RAII reference to a block
class Ref {
  public:
    Ref() = default;
    Ref(Engine *e, Bid id) : e_(e), id_(id) {}   // adopts one reference
    Ref(const Ref &o) : e_(o.e_), id_(o.id_) { if (id_) e_->retain(id_); }
    Ref(Ref &&o) noexcept : e_(o.e_), id_(o.id_) { o.id_ = 0; }
    Ref &operator=(Ref o) noexcept { std::swap(e_, o.e_); std::swap(id_, o.id_); return *this; }
    ~Ref() { if (id_) e_->release(id_); }
    Bid id() const { return id_; }
    Engine *engine() const { return e_; }
    Bid detach() { Bid t = id_; id_ = 0; return t; }   // caller takes the reference
    explicit operator bool() const { return id_ != 0; }

  private:
    Engine *e_ = nullptr;
    Bid id_ = 0;
};

}  // namespace fhs
