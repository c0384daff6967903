// CPU restatement of the four per-point formulas of the scan filters that follow kNN and covariances (csrc/scan_refine.hip),
// written for this project's tests from the formulas as DESIGN.md section 4.7 states them:
//   angle of incidence   keep = finite(p) && denom > 1e-6f && cos(max_angle) <= |p.n / denom| <= cos(min_angle),
//                        p.n an fma chain from 0, denom = |p| |n| with each norm the square root of such a chain
//   intensity correction I' = clamp(I * pow(|p| / ref, e) * angle_factor * scale, lo, hi), |p| from plain products and sums,
//                        angle_factor = pow(max(|cos|, 1e-3f), -a), or 1 (no normals, a == 0, denom <= 1e-6f)
//   Gaussian smoothing   sum w I / sum w over the listed neighbours, w = exp(-(dr^2 i_r + daz^2 i_az + del^2 i_el)) in the
//                        sensor-local basis (radial, azimuthal tangent, elevation tangent; x / y axes near the zenith)
//   local-mean norm      I / fmax(that mean, mean_min)
// Compile with -ffp-contract=off: the only fused operations are the std::fma written here. Every function exists twice: *_restate
// evaluates in float, *_f64 evaluates the same formula in double from the same float inputs (thresholds are the float constants).
// A neighbour index outside [0, n) is skipped, as the library skips it.
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

template <class T>
T chain3(T a0, T b0, T a1, T b1, T a2, T b2) {
    return std::fma(a2, b2, std::fma(a1, b1, std::fma(a0, b0, T(0))));
}

// |cos| of the angle between p and nr; false when the denominator is too small for one
template <class T>
bool abs_cos_of(const float* p, const float* nr, T& abs_cos) {
    const T px = p[0], py = p[1], pz = p[2], nx = nr[0], ny = nr[1], nz = nr[2];
    const T dot = chain3<T>(px, nx, py, ny, pz, nz);
    const T denom = std::sqrt(chain3<T>(px, px, py, py, pz, pz)) * std::sqrt(chain3<T>(nx, nx, ny, ny, nz, nz));
    if (denom <= T(1e-6f)) return false;
    abs_cos = std::fabs(dot / denom);
    return true;
}

template <class T>
void angle_flags(const float* points, const float* normals, uint64_t n, float min_angle, float max_angle, uint8_t* flags) {
    // the cosines are formed once, in float, by the host in both modes: they are inputs of the kernel
    const T max_cos = std::cos(min_angle), min_cos = std::cos(max_angle);
    for (uint64_t i = 0; i < n; ++i) {
        const float* p = points + 4 * i;
        flags[i] = 0;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]))) continue;
        T c;
        if (!abs_cos_of<T>(p, normals + 4 * i, c)) continue;
        flags[i] = !(c < min_cos || c > max_cos);
    }
}

template <class T>
void intensity_correct(const float* points, const float* normals, const float* in, uint64_t n, float exponent, float scale,
                       float lo, float hi, float ref_distance, float angle_exponent, T* out) {
    const bool use_angle = normals && angle_exponent != 0.0f;
    for (uint64_t i = 0; i < n; ++i) {
        const float* p = points + 4 * i;
        T angle_factor = 1;
        T c;
        if (use_angle && abs_cos_of<T>(p, normals + 4 * i, c))
            angle_factor = std::pow(std::fmax(c, T(1e-3f)), -T(angle_exponent));
        const T x = p[0], y = p[1], z = p[2];
        const T dist = std::sqrt(x * x + y * y + z * z);
        const T dist_factor = std::pow(dist / T(ref_distance), T(exponent));
        out[i] = std::fmin(std::fmax(T(in[i]) * dist_factor * angle_factor * T(scale), T(lo)), T(hi));
    }
}

// row_min_exp / row_max_exp (may be null): the smallest / largest exponent among the neighbours of row i that were used
// (+inf / -inf when none was)
template <class T>
void intensity_gaussian(const float* points, const float* in, const int32_t* knn, uint64_t n, uint64_t k_stride, uint64_t k_use,
                        float s_az, float s_el, float s_r, float mean_min, T* out, double* row_min_exp, double* row_max_exp) {
    const T inv2_az = T(0.5f) / (T(s_az) * T(s_az)), inv2_el = T(0.5f) / (T(s_el) * T(s_el)), inv2_r = T(0.5f) / (T(s_r) * T(s_r));
    for (uint64_t i = 0; i < n; ++i) {
        const T px = points[4 * i], py = points[4 * i + 1], pz = points[4 * i + 2];
        const T own = in[i];
        T mean = own;
        double lo = INFINITY, hi = -INFINITY;
        const T r = std::sqrt(px * px + py * py + pz * pz);
        if (!(r < T(1e-6f))) {
            const T rx = px / r, ry = py / r, rz = pz / r;
            const T rxy = std::sqrt(px * px + py * py);
            const bool zenith = rxy < T(1e-6f);
            const T inv_rxy = T(1) / std::fmax(rxy, T(1e-6f));
            const T ax = zenith ? T(1) : (-py * inv_rxy), ay = zenith ? T(0) : (px * inv_rxy);
            const T ex = zenith ? T(0) : (-rz * ay), ey = zenith ? T(1) : (rz * ax), ez = zenith ? T(0) : (rxy / r);
            T sum_w = 0, sum_wI = 0;
            for (uint64_t j = 0; j < k_use; ++j) {
                const int64_t idx = knn[i * k_stride + j];
                if (idx < 0 || (uint64_t)idx >= n) continue;
                const T dx = T(points[4 * idx]) - px, dy = T(points[4 * idx + 1]) - py, dz = T(points[4 * idx + 2]) - pz;
                const T d_r = dx * rx + dy * ry + dz * rz;
                const T d_az = dx * ax + dy * ay;
                const T d_el = dx * ex + dy * ey + dz * ez;
                const T e = d_r * d_r * inv2_r + d_az * d_az * inv2_az + d_el * d_el * inv2_el;
                const T w = std::exp(-e);
                sum_w += w;
                sum_wI += w * T(in[idx]);
                if ((double)e < lo) lo = (double)e;
                if ((double)e > hi) hi = (double)e;
            }
            mean = sum_w > T(0) ? sum_wI / sum_w : own;
        }
        out[i] = mean_min > 0.0f ? own / std::fmax(mean, T(mean_min)) : mean;
        if (row_min_exp) row_min_exp[i] = lo;
        if (row_max_exp) row_max_exp[i] = hi;
    }
}

}  // namespace

extern "C" {
void angle_flags_restate(const float* p, const float* nr, uint64_t n, float a0, float a1, uint8_t* f) { angle_flags<float>(p, nr, n, a0, a1, f); }
void angle_flags_f64(const float* p, const float* nr, uint64_t n, float a0, float a1, uint8_t* f) { angle_flags<double>(p, nr, n, a0, a1, f); }
void intensity_correct_restate(const float* p, const float* nr, const float* in, uint64_t n, float e, float s, float lo, float hi,
                               float ref, float a, float* out) {
    intensity_correct<float>(p, nr, in, n, e, s, lo, hi, ref, a, out);
}
void intensity_correct_f64(const float* p, const float* nr, const float* in, uint64_t n, float e, float s, float lo, float hi,
                           float ref, float a, double* out) {
    intensity_correct<double>(p, nr, in, n, e, s, lo, hi, ref, a, out);
}
void intensity_gaussian_restate(const float* p, const float* in, const int32_t* knn, uint64_t n, uint64_t ks, uint64_t ku, float s_az,
                                float s_el, float s_r, float mean_min, float* out, double* emin, double* emax) {
    intensity_gaussian<float>(p, in, knn, n, ks, ku, s_az, s_el, s_r, mean_min, out, emin, emax);
}
void intensity_gaussian_f64(const float* p, const float* in, const int32_t* knn, uint64_t n, uint64_t ks, uint64_t ku, float s_az,
                            float s_el, float s_r, float mean_min, double* out, double* emin, double* emax) {
    intensity_gaussian<double>(p, in, knn, n, ks, ku, s_az, s_el, s_r, mean_min, out, emin, emax);
}
}
