#include "hip_owners.h"

#include <atomic>

namespace fhs {

namespace {
enum { DEV_BYTES, PINNED_BYTES, EVENTS, STREAMS, ACQUIRED, N_FIGURES };
std::atomic<uint64_t> g_live[N_FIGURES];
constexpr auto RELAXED = std::memory_order_relaxed;
void took(int what, uint64_t n) {
    g_live[what].fetch_add(n, RELAXED);
    g_live[ACQUIRED].fetch_add(1, RELAXED);
}
}  // namespace

void live_resources(uint64_t out[5]) {
    for (int k = 0; k < N_FIGURES; k++) out[k] = g_live[k].load(RELAXED);
}

template <Mem M> hipError_t Buf<M>::reserve_exact(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = M == Mem::Device ? hipMalloc(&ptr, bytes) : hipHostMalloc(&ptr, bytes, hipHostMallocDefault);
    if (e == hipSuccess) { cap = bytes; took((int)M, bytes); }
    else ptr = nullptr;
    return e;
}
template <Mem M> void Buf<M>::release() {
    if (ptr) {
        (void)(M == Mem::Device ? hipFree(ptr) : hipHostFree(ptr));
        g_live[(int)M].fetch_sub(cap, RELAXED);
    }
    ptr = nullptr;
    cap = 0;
}
template struct Buf<Mem::Device>;
template struct Buf<Mem::Pinned>;
static_assert((int)Mem::Device == DEV_BYTES && (int)Mem::Pinned == PINNED_BYTES, "figure order");

hipEvent_t Event::get() {
    if (!e_) {
        if (hipEventCreateWithFlags(&e_, flags_) == hipSuccess) took(EVENTS, 1);
        else e_ = nullptr;
    }
    return e_;
}
void Event::reset() {
    if (e_) { (void)hipEventDestroy(e_); g_live[EVENTS].fetch_sub(1, RELAXED); }
    e_ = nullptr;
}

hipError_t Stream::create(const uint32_t *cu_mask, uint32_t n_words) {
    destroy();
    hipError_t e = cu_mask ? hipExtStreamCreateWithCUMask(&s_, n_words, cu_mask) : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    if (e == hipSuccess) took(STREAMS, 1);
    else s_ = nullptr;
    return e;
}
void Stream::destroy() {
    if (s_) { (void)hipStreamDestroy(s_); g_live[STREAMS].fetch_sub(1, RELAXED); }
    s_ = nullptr;
}

}  // namespace fhs
