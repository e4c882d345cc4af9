// What an Engine holds on the device besides its DAG: the block pool and the transfer buffer of whole-string uploads
// and downloads, each built on the owners of hip_owners.h.
#pragma once
#include <map>
#include <vector>

#include "hip_owners.h"

namespace fhs {

// Device block pool: blocks of 2050 words (16-byte aligned rows) carved from chunks of 2048 blocks (33.6 MB).  On a
// planner context it hands out distinct non-null tokens that are never dereferenced.
class BlockPool {
  public:
    explicit BlockPool(const bool &planner) : planner_(planner) {}
    uint64_t *alloc() {                                  // nullptr: the device is out of memory
        if (planner_) {
            live_++;
            return reinterpret_cast<uint64_t *>((uintptr_t)0x1000 + 8 * (uintptr_t)(++tokens_));
        }
        if (free_.empty() && !grow()) return nullptr;
        uint64_t *p = free_.back();
        free_.pop_back();
        live_++;
        return p;
    }
    // A scheduled job level that has not been enqueued yet may still read the block (last_sched_tick >= next_tick): it
    // becomes reusable once every tick scheduled so far is in the stream -- stream order then protects the readers.
    void free(uint64_t *p, uint64_t last_sched_tick, uint64_t next_tick) {
        if (!planner_) {
            if (last_sched_tick >= next_tick) free_after_[last_sched_tick].push_back(p);
            else free_.push_back(p);
        }
        live_--;
    }
    void tick_enqueued(uint64_t tick);                   // blocks freed while ticks <= `tick` were pending are reusable now
    uint64_t live() const { return live_; }

    static constexpr size_t STRIDE = 2050, CHUNK_BLOCKS = 2048;   // u64 words per block, blocks per hipMalloc
    static constexpr size_t CHUNK_BYTES = CHUNK_BLOCKS * STRIDE * 8;
    // ---- accounting and trimming (fhs_pool_stats / fhs_pool_trim) ----
    // [chunks, CHUNK_BLOCKS, live, free, freed under a scheduled tick and not reusable yet, device bytes of the chunks];
    // a planner holds no chunk: [0, CHUNK_BLOCKS, live, 0, 0, 0]
    void stats(uint64_t out[6]) const;
    // The victim choice, a pure function of the occupancies: the pool keeps K = ceil((live + keep_free_blocks) / 2048)
    // chunks, the victims are the n_chunks - K chunks with the fewest live blocks, ties going to the chunk allocated last.
    static void plan_trim(const uint32_t *live_per_chunk, size_t n_chunks, size_t keep_free_blocks, uint8_t *victim);
    size_t n_chunks() const { return chunks_.size(); }
    uint64_t *slot_ptr(size_t chunk, size_t slot) const { return chunks_[chunk].as<uint64_t>() + slot * STRIDE; }
    // chunk (in allocation order) and slot of every pointer; false: one of them is no block of this pool
    bool locate(uint64_t *const *p, size_t n, uint32_t *chunk, uint32_t *slot) const;
    // Gives the victims back: free_ loses their slots and the slots marked in used[chunk * CHUNK_BLOCKS + slot] (the
    // destinations of a compaction) and keeps its order otherwise; then the victims' allocations are destroyed.  The
    // caller has waited for the stream and no victim holds a live block any more.  -> bytes given back
    uint64_t release(const std::vector<uint8_t> &victim, const std::vector<uint8_t> &used);

  private:
    bool grow();
    const bool &planner_;
    std::vector<DevBuf> chunks_;
    std::vector<uint64_t *> free_;
    std::map<uint64_t, std::vector<uint64_t *>> free_after_;
    uint64_t live_ = 0, tokens_ = 0;
};

// Pinned host buffer + device mirror for rows of 2049 words and their pointer table, shared by every whole-string
// upload, read_many and store_get.  Its two rules live here: the host waits for the last copy out of the pinned side
// before writing it again, and a buffer that grows first waits for that copy and for the stream (queued kernels read
// the old mirror).
class TransferBuffer {
  public:
    uint64_t *pin() const { return pin_.as<uint64_t>(); }
    uint64_t *dev() const { return dev_.as<uint64_t>(); }
    bool ensure(size_t rows, hipStream_t s);             // room for `rows` rows and their pointers, at least 260
    // a pass that writes the buffer from word 0: room for `rows` rows (0: the minimum size), the last copy has left it
    bool begin_pass(size_t rows, hipStream_t s);
    // A pass that sends `n` words ALONE (a pointer table, store_get): consecutive passes take consecutive segments
    // [at, at + n) of both sides, so the host only waits when the buffer wraps or after a pass of the other kind.  The
    // copy of a table is queued behind everything on the stream, a whole launch group included: waiting for the previous
    // table before writing the next one would tie a caller that restores string k + 1 while the GPU works on string k
    // (fhs_submit / fhs_pump) to the GPU's pace.
    bool begin_table_pass(size_t n, size_t &at, hipStream_t s);
    hipError_t copy_up(size_t at, size_t words, hipStream_t s);   // pinned [at, at + words) -> mirror; records the event

  private:
    static constexpr size_t CURSOR_RESET = ~(size_t)0;
    PinnedBuf pin_;
    DevBuf dev_;
    size_t words_ = 0;                                   // of either side
    Event done_{hipEventDisableTiming};                  // behind the last copy_up
    size_t cursor_ = CURSOR_RESET;                       // next free word for a table pass
};

}  // namespace fhs
