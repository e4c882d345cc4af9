// Owners of the HIP resources this library acquires: one object per device allocation, pinned host allocation, event
// and stream.  An owner is movable (the source is left empty), not copyable, makes no HIP call while it holds nothing
// (planner contexts and the sanitizer driver run without a device), gives back what it holds when it dies, and is
// counted (live_resources).  No other file under csrc/ allocates, creates or destroys one of these.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace fhs {

enum class Mem { Device, Pinned };   // hipMalloc / hipHostMalloc

// one allocation, grow-only
template <Mem M> struct Buf {
    void *ptr = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) { release(); ptr = o.ptr; cap = o.cap; o.ptr = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { release(); }
    // scratch: at least 1 MB, so that a growing batch does not reallocate often
    hipError_t reserve(size_t bytes) { return bytes <= cap ? hipSuccess : reserve_exact(bytes > ((size_t)1 << 20) ? bytes : (size_t)1 << 20); }
    hipError_t reserve_exact(size_t bytes);   // key material, tables, the work counter, staging: sizes the caller chose
    void release();
    explicit operator bool() const { return ptr != nullptr; }
    template <class T> T *as() const { return reinterpret_cast<T *>(ptr); }
};
using DevBuf = Buf<Mem::Device>;
using PinnedBuf = Buf<Mem::Pinned>;

// one event, created on first use with the flags chosen at construction (hipEventDisableTiming for a guard, the
// default for the kernel timer)
class Event {
  public:
    explicit Event(unsigned flags = hipEventDefault) : flags_(flags) {}
    Event(Event &&o) noexcept : e_(o.e_), flags_(o.flags_) { o.e_ = nullptr; }
    Event &operator=(Event &&o) noexcept {
        if (this != &o) { reset(); e_ = o.e_; flags_ = o.flags_; o.e_ = nullptr; }
        return *this;
    }
    ~Event() { reset(); }
    hipEvent_t get();                          // creates it if need be; nullptr: the creation failed
    hipEvent_t peek() const { return e_; }     // nullptr until get() has created it
    void reset();

  private:
    hipEvent_t e_ = nullptr;
    unsigned flags_;
};

// one non-blocking stream; converts to the hipStream_t it holds (nullptr before create)
class Stream {
  public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { destroy(); }
    hipError_t create(const uint32_t *cu_mask = nullptr, uint32_t n_words = 0);   // a mask: hipExtStreamCreateWithCUMask
    void destroy();
    operator hipStream_t() const { return s_; }

  private:
    hipStream_t s_ = nullptr;
};

// fhs_debug_live_resources: [device bytes, pinned bytes, events, streams] the owners of this process hold now, and the
// acquisitions since process start
void live_resources(uint64_t out[5]);

}  // namespace fhs
