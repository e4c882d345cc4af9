// The one host-thread fan-out of the library (key generation, key conversion, string encryption, host references).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <thread>
#include <vector>

namespace fhs {

// Host threads a loop may use: what the machine reports, at most `cap`, at least one.  The only caller of
// hardware_concurrency(): a policy for machines that grant a process fewer CPUs than they report belongs here.
inline unsigned host_threads(unsigned cap) { return std::max(1u, std::min(cap, std::thread::hardware_concurrency())); }

// f(i) for every i in [0, n) on at most `max_threads` threads, the caller among them; the items are handed out `grain`
// at a time from one counter, in no fixed order.  Every caller's item writes only its own slice of the output and draws
// only from generator streams named by its own index, so the result does not depend on the thread count or the order.
template <class F>
void parallel_for(size_t n, size_t max_threads, size_t grain, F &&f) {
    const size_t nt = std::min(max_threads, (n + grain - 1) / grain);
    if (nt <= 1) {
        for (size_t i = 0; i < n; i++) f(i);
        return;
    }
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i0; (i0 = next.fetch_add(grain)) < n;)
            for (size_t i = i0; i < std::min(n, i0 + grain); i++) f(i);
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &x : th) x.join();
}

}  // namespace fhs
