// CPU restatement of the three formulas of csrc/outlier.hip, written for this project's tests from the formulas as DESIGN.md
// section 4.11 states them:
//   statistical outliers  m[i] = (d[i][0] + ... + d[i][k_use-1]) / k_use over a row of SQUARED neighbour distances, in index order;
//                         g = sum m / n; var = sum (g - m)^2 / n; thr = g + mul * sqrt(var); keep = !(m > thr)
//   radius outliers       keep = !(d[i][column] > radius): the squared distance against the radius itself
//   intensity z-score     over the first k_use listed neighbours, in index order: S = sum I, Q = sum I * I; mean = S / k_use;
//                         var = fmax(Q / k_use - mean * mean, 0); sigma = sqrt(var); 0 when sigma < sigma_min, else
//                         (I[i] - mean) / sigma. A neighbour index outside [0, n) adds nothing; the divisor stays k_use.
// Compile with -ffp-contract=off: every product and sum is one rounding. Every function exists twice: *_restate evaluates in float
// with every sum taken sequentially in index order (the row sums, and the two sums over the points too), *_f64 evaluates the same
// formula in double from the same float inputs (sigma_min, radius and mul are the float constants).
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

// stats: {g, var, thr, n}
template <class T>
void statistical(const float* d2, uint64_t n, uint64_t k_stride, uint64_t k_use, float mul, T* mean, T* stats, uint8_t* flags) {
    const T kf = T(k_use), nf = T(n);
    T total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        T row = 0;
        for (uint64_t j = 0; j < k_use; ++j) row += T(d2[i * k_stride + j]);
        mean[i] = row / kf;
        total += mean[i];
    }
    const T g = total / nf;
    T spread = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const T sub = g - mean[i];
        spread += sub * sub;
    }
    const T var = spread / nf;
    const T thr = g + T(mul) * std::sqrt(var);
    for (uint64_t i = 0; i < n; ++i) flags[i] = mean[i] > thr ? 0 : 1;
    stats[0] = g;
    stats[1] = var;
    stats[2] = thr;
    stats[3] = nf;
}

template <class T>
void zscore(const float* intensities, const int32_t* knn, uint64_t n, uint64_t k_stride, uint64_t k_use, float sigma_min, T* out) {
    const T kf = T(k_use);
    for (uint64_t i = 0; i < n; ++i) {
        T s = 0, q = 0;
        for (uint64_t j = 0; j < k_use; ++j) {
            const int64_t idx = knn[i * k_stride + j];
            if (idx < 0 || uint64_t(idx) >= n) continue;
            const T v = intensities[idx];
            s += v;
            q += v * v;
        }
        const T mean = s / kf;
        const T var = std::fmax(q / kf - mean * mean, T(0));
        const T sigma = std::sqrt(var);
        out[i] = sigma < T(sigma_min) ? T(0) : (T(intensities[i]) - mean) / sigma;
    }
}

}  // namespace

extern "C" {

void outlier_statistical_restate(const float* d2, uint64_t n, uint64_t k_stride, uint64_t k_use, float mul, float* mean, float* stats,
                                 uint8_t* flags) {
    statistical<float>(d2, n, k_stride, k_use, mul, mean, stats, flags);
}
void outlier_statistical_f64(const float* d2, uint64_t n, uint64_t k_stride, uint64_t k_use, float mul, double* mean, double* stats,
                             uint8_t* flags) {
    statistical<double>(d2, n, k_stride, k_use, mul, mean, stats, flags);
}
// the comparison involves no arithmetic: one function serves both precisions
void outlier_radius_restate(const float* d2, uint64_t n, uint64_t k_stride, uint64_t column, float radius, uint8_t* flags) {
    for (uint64_t i = 0; i < n; ++i) flags[i] = d2[i * k_stride + column] > radius ? 0 : 1;
}
void intensity_zscore_restate(const float* intensities, const int32_t* knn, uint64_t n, uint64_t k_stride, uint64_t k_use,
                              float sigma_min, float* out) {
    zscore<float>(intensities, knn, n, k_stride, k_use, sigma_min, out);
}
void intensity_zscore_f64(const float* intensities, const int32_t* knn, uint64_t n, uint64_t k_stride, uint64_t k_use, float sigma_min,
                          double* out) {
    zscore<double>(intensities, knn, n, k_stride, k_use, sigma_min, out);
}
}
