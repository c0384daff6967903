// CPU restatement of the reference's farthest point sampling (filter/preprocess_operator/farthest_point_sampling_operator.hpp:
// 27-91), for the FPS tests: built by tests/test_fps_cpu.py with g++ -O2 -ffp-contract=off as a shared library and loaded by
// ctypes. It is the reference's loop written out on the host, one rule per line:
//   first index   std::uniform_int_distribution<size_t>(0, N - 1) on a std::mt19937 (:51-53; seeded 1234 at construction)
//   distance      frobenius_norm_squared<4>(subtract<4,1>(p[gid], p[sel])): dot<4> = fma(dw,dw, fma(dz,dz, fma(dy,dy,
//                 fma(dx,dx, 0)))) (utils/eigen_utils.hpp:245-253, :333-335)
//   update        d[gid] = sycl::min(d[gid], dist) = (dist < d[gid]) ? dist : d[gid] (:71)
//   argmax        std::max_element: the first maximum (:77-83)
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <random>
#include <vector>

extern "C" {

// The reference's first index for a cloud of n points, the `draws`-th draw (1 = the first) of a generator seeded with `seed`.
uint64_t fps_first_index(uint32_t seed, uint64_t n, int draws) {
    std::mt19937 mt(seed);
    uint64_t r = 0;
    for (int k = 0; k < draws; ++k) {
        std::uniform_int_distribution<size_t> dist(0, n - 1);
        r = dist(mt);
    }
    return r;
}

// order[0..S) and d[0..n) after sampling S points from `first` (S >= 1); points: float4[n].
void fps_restate(const float* points, uint64_t n, uint64_t S, uint64_t first, uint32_t* order, float* d) {
    for (uint64_t i = 0; i < n; ++i) d[i] = std::numeric_limits<float>::max();
    uint64_t sel = first;
    order[0] = (uint32_t)sel;
    for (uint64_t it = 1; it < S; ++it) {
        const float* s = points + 4 * sel;
        for (uint64_t i = 0; i < n; ++i) {
            const float* p = points + 4 * i;
            const float dx = p[0] - s[0], dy = p[1] - s[1], dz = p[2] - s[2], dw = p[3] - s[3];
            const float dist = std::fmaf(dw, dw, std::fmaf(dz, dz, std::fmaf(dy, dy, std::fmaf(dx, dx, 0.0f))));
            d[i] = (dist < d[i]) ? dist : d[i];
        }
        uint64_t best = 0;
        for (uint64_t i = 1; i < n; ++i)
            if (d[i] > d[best]) best = i;  // (strictly greater: the first maximum stays)
        sel = best;
        order[it] = (uint32_t)sel;
    }
}
}
