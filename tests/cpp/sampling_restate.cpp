// CPU restatement of the reference's weighted and mixed random samplers (filter/preprocess_operator/
// weighted_sampling_operator.hpp:29-95, mixed_random_sampling_operator.hpp:28-105), for the sampling tests: built by
// tests/test_sampling_cpu.py with g++ -O2 -ffp-contract=off as a shared library and loaded by ctypes (tests/cpp/test_sampling.cpp
// includes it). The two operators are written out on the host as the reference has them, one rule per line:
//   small    N <= sampling_num keeps every point, before any check
//   checks   weighted: a weight not finite or < 0, no positive weight, sampling_num > positive weights (in this order);
//            mixed: weighted_ratio not finite or outside [0, 1], then (inside the loop) a weight not finite or < 0
//   key      std::log(u) / w in float, u = std::uniform_real_distribution<float>(FLT_MIN, 1.0f) on a std::mt19937, one draw per
//            positive weight in index order (mixed: none at all when the share drawn by weight is 0)
//   heap     std::priority_queue of (key, index) with std::greater: the smallest pair on top; filled up to the target, then
//            the top is replaced only when top.key < key
//   uniform  (mixed) a partial Fisher-Yates over the unselected indices, ascending, std::uniform_int_distribution<size_t>(i, R - 1)
//            on the SAME generator, after the weighted draws
// Return codes of the two operators: 0 done, else the number of the check that threw (1 a bad weight, 2 no positive weight,
// 3 sampling_num above the positive weights, 4 a bad ratio).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <limits>
#include <queue>
#include <random>
#include <unordered_map>
#include <utility>
#include <vector>

namespace sampling_restate {

// one kept point: its key first, so that pairs order by key and then by index
using Entry = std::pair<float, size_t>;
// the smallest entry on top
using KeptHeap = std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>>;

// One point arrives: it enters while fewer than `room` are kept; afterwards it replaces the top only when the top's key is
// strictly smaller. (`room` is at least 1 wherever this is called.)
inline void heap_step(KeptHeap& kept, size_t room, float key, size_t index) {
    if (kept.size() < room) {
        kept.emplace(key, index);
    } else if (kept.top().first < key) {
        kept.pop();
        kept.emplace(key, index);
    }
}

inline void heap_to_flags(KeptHeap& kept, uint8_t* flags) {
    for (; !kept.empty(); kept.pop()) flags[kept.top().second] = 1;
}

inline bool bad_weight(float w) { return !std::isfinite(w) || w < 0.0f; }

inline int weighted(std::mt19937& mt, const float* weights, size_t N, size_t sampling_num, uint8_t* flags) {
    if (N <= sampling_num) {
        std::fill(flags, flags + N, uint8_t(1));
        return 0;
    }
    size_t positive = 0;
    for (size_t i = 0; i < N; ++i) {
        if (bad_weight(weights[i])) return 1;
        positive += weights[i] > 0.0f ? 1 : 0;
    }
    if (positive == 0) return 2;
    if (sampling_num > positive) return 3;
    std::fill(flags, flags + N, uint8_t(0));
    KeptHeap kept;
    std::uniform_real_distribution<float> draw(std::numeric_limits<float>::min(), 1.0f);
    for (size_t i = 0; i < N; ++i) {
        const float w = weights[i];
        if (!(w > 0.0f)) continue;
        heap_step(kept, sampling_num, std::log(draw(mt)) / w, i);
    }
    heap_to_flags(kept, flags);
    return 0;
}

inline int mixed(std::mt19937& mt, const float* weights, size_t N, size_t sampling_num, float weighted_ratio, uint8_t* flags) {
    if (N <= sampling_num) {
        std::fill(flags, flags + N, uint8_t(1));
        return 0;
    }
    if (!std::isfinite(weighted_ratio) || weighted_ratio < 0.0f || weighted_ratio > 1.0f) return 4;
    const size_t by_weight = size_t(std::floor(double(sampling_num) * double(weighted_ratio)));
    std::fill(flags, flags + N, uint8_t(0));
    KeptHeap kept;
    std::uniform_real_distribution<float> draw(std::numeric_limits<float>::min(), 1.0f);
    for (size_t i = 0; i < N; ++i) {
        const float w = weights[i];
        if (bad_weight(w)) return 1;  // (met inside the loop: the positive weights before it have drawn)
        if (by_weight == 0 || !(w > 0.0f)) continue;
        heap_step(kept, by_weight, std::log(draw(mt)) / w, i);
    }
    heap_to_flags(kept, flags);
    std::vector<size_t> open;  // the points not kept so far, ascending
    open.reserve(N);
    for (size_t i = 0; i < N; ++i)
        if (flags[i] != 1) open.push_back(i);
    const size_t by_chance = std::min(sampling_num - (N - open.size()), open.size());
    for (size_t i = 0; i < by_chance; ++i) {  // partial Fisher-Yates on the same generator
        const size_t j = std::uniform_int_distribution<size_t>(i, open.size() - 1)(mt);
        std::swap(open[i], open[j]);
        flags[open[i]] = 1;
    }
    return 0;
}

}  // namespace sampling_restate

extern "C" {

// The two operators with a generator seeded `seed`. flags: u8[N], 1 keep / 0 remove.
int sampling_weighted_restate(uint32_t seed, const float* weights, uint64_t N, uint64_t sampling_num, uint8_t* flags) {
    std::mt19937 mt(seed);
    return sampling_restate::weighted(mt, weights, N, sampling_num, flags);
}
int sampling_mixed_restate(uint32_t seed, const float* weights, uint64_t N, uint64_t sampling_num, float weighted_ratio,
                           uint8_t* flags) {
    std::mt19937 mt(seed);
    return sampling_restate::mixed(mt, weights, N, sampling_num, weighted_ratio, flags);
}

// The first `count` weighted draws of a generator seeded `seed`.
void sampling_draws(uint32_t seed, uint64_t count, float* u) {
    std::mt19937 mt(seed);
    std::uniform_real_distribution<float> dist(std::numeric_limits<float>::min(), 1.0f);
    for (uint64_t j = 0; j < count; ++j) u[j] = dist(mt);
}

// keys[i] = std::log(u of the point's rank among the positive weights) / w, NaN for a weight that is not positive.
void sampling_keys(const float* weights, const float* u_by_rank, uint64_t N, float* keys) {
    uint64_t j = 0;
    for (uint64_t i = 0; i < N; ++i)
        keys[i] = weights[i] > 0.0f ? std::log(u_by_rank[j++]) / weights[i] : std::numeric_limits<float>::quiet_NaN();
}

// The heap alone on given keys (NaN: no key, the point is skipped): flags of the `m` kept. The tie rule's literal form.
void sampling_heap_select(const float* keys, uint64_t N, uint64_t m, uint8_t* flags) {
    std::fill(flags, flags + N, uint8_t(0));
    sampling_restate::KeptHeap kept;
    for (uint64_t i = 0; i < N; ++i)
        if (!std::isnan(keys[i])) sampling_restate::heap_step(kept, m, keys[i], i);
    sampling_restate::heap_to_flags(kept, flags);
}

// The positions, in the ascending list of R unselected points, that the partial Fisher-Yates selects: U draws of a generator
// seeded `seed` that has made `weighted_draws` weighted draws before. The list is held as a sparse map of its swapped slots.
void sampling_uniform_positions(uint32_t seed, uint64_t weighted_draws, uint64_t R, uint64_t U, uint64_t* positions) {
    std::mt19937 mt(seed);
    std::uniform_real_distribution<float> dist(std::numeric_limits<float>::min(), 1.0f);
    for (uint64_t j = 0; j < weighted_draws; ++j) (void)dist(mt);
    std::unordered_map<size_t, size_t> moved;
    auto at = [&](size_t k) { auto it = moved.find(k); return it == moved.end() ? k : it->second; };
    for (size_t i = 0; i < U; ++i) {
        const size_t j = std::uniform_int_distribution<size_t>(i, R - 1)(mt);
        const size_t vi = at(i), vj = at(j);
        moved[i] = vj;
        moved[j] = vi;
        positions[i] = vj;
    }
}
}
