// The registry of user tables (luts.h): process-wide, append-only, interned by content.
#include "luts.h"

#include <array>
#include <atomic>
#include <map>
#include <mutex>

namespace fhs {

namespace {
// readers (lut_function on every folded bootstrap) take no lock: an entry is written once, before the count that
// publishes it (release / acquire), and never again
uint8_t g_values[USER_LUT_CAPACITY][16];
std::atomic<int> g_count{0};
std::mutex g_mutex;
std::map<std::array<uint8_t, 16>, int> g_by_content;
}  // namespace

int user_lut_register(const uint8_t values[16]) {
    std::array<uint8_t, 16> key;
    for (int i = 0; i < 16; i++) key[i] = values[i] & 31;
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = g_by_content.find(key);
    if (it != g_by_content.end()) return it->second;
    const int n = g_count.load(std::memory_order_relaxed);
    if (n >= USER_LUT_CAPACITY) return -1;
    for (int i = 0; i < 16; i++) g_values[n][i] = key[i];
    g_by_content.emplace(key, LUT_COUNT + n);
    g_count.store(n + 1, std::memory_order_release);
    return LUT_COUNT + n;
}

int user_lut_count() { return g_count.load(std::memory_order_acquire); }

const uint8_t *user_lut_values(int id) {
    const int k = id - LUT_COUNT;
    return k >= 0 && k < g_count.load(std::memory_order_acquire) ? g_values[k] : nullptr;
}

}  // namespace fhs
