// The scan filters that follow kNN and covariances, for gfx950 (the reference's refine_filter stage,
// pipeline/pointcloud_processing.hpp:158-203):
//   sp_angle_incidence_flags  AngleIncidenceFilterOperator::apply   (filter/preprocess_operator/angle_incidence_filter_operator.hpp:23-110)
//   sp_intensity_correct      intensity_correction::correct_intensity (filter/intensity_correction.hpp:20-135)
//   sp_intensity_gaussian     intensity_gaussian::kernel::compute     (filter/intensity_gaussian.hpp:37-86) and
//                             intensity_local_mean_norm::kernel::compute (filter/intensity_local_mean_norm.hpp:26-32)
//
// One lane per point with a grid-stride loop, no LDS, no cross-lane work. dot<3> and frobenius_norm<3> are sp_math.h's chain3
// (eigen_utils.hpp:245-253, 333-354: fma chains from 0); everything the reference writes as a plain product or sum stays one
// (the file is compiled with -ffp-contract=off). sqrt and division are correctly rounded (hipcc's default). The normal of a
// covariance is sp_cov_normal.h's normal_of, the function sp_normals_from_cov stores: the covariance paths carry the bits the
// normal paths get from its output.
//
// Bytes per point (every access 16 bytes wide except the flag byte, the intensity and the index row of an odd stride):
//   angle flags       normals 16 + 16 + 1 = 33      covs 16 + 48 + 1 = 65   (three columns of the covariance)
//   intensity correct none 16 + 4 + 4 = 24          normals 40          covs 72
//   gaussian / local mean   4 k (index row) + 20 k (gathered point + intensity) + 20 (own) + 4 (store): 264 at k = 10
// The gather is K5's shape (covariance.hip): the index row is contiguous per lane, the k points and intensities are random
// 16- and 4-byte reads out of L2 / Infinity Cache. With k_stride a multiple of 4 a lane reads its row as 16-byte words.
#include <cmath>
#include <cstdio>

#include "sp_common.h"
#include "sp_math.h"
#include "sp_cov_normal.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

enum { kNoAngle = 0, kFromNormals = 1, kFromCovs = 2 };

__device__ __forceinline__ bool finite4(const float4 p) {  // preprocess_operator/common.hpp:15-17
    return fabsf(p.x) <= FLT_MAX && fabsf(p.y) <= FLT_MAX && fabsf(p.z) <= FLT_MAX && fabsf(p.w) <= FLT_MAX;
}

// dot<3>(p, n) and ||p|| * ||n|| as compute_flag / compute_angle_factor form them
__device__ __forceinline__ void dot_and_denom(const float4 p, const float4 nr, float& dot, float& denom) {
    dot = chain3(p.x, nr.x, p.y, nr.y, p.z, nr.z);
    denom = sqrtf(chain3(p.x, p.x, p.y, p.y, p.z, p.z)) * sqrtf(chain3(nr.x, nr.x, nr.y, nr.y, nr.z, nr.z));
}

template <int SRC>  // kFromNormals | kFromCovs
__global__ __launch_bounds__(kBlock) void angle_flags_kernel(const float4* __restrict__ points, const float4* __restrict__ normals,
                                                             const float4* __restrict__ covs, unsigned n, float min_cos,
                                                             float max_cos, uint8_t* __restrict__ flags) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 p = points[i];
        uint8_t keep = 0;
        if (finite4(p)) {
            const float4 nr = SRC == kFromCovs ? normal_of(load_cov(covs + 4 * (size_t)i), p) : normals[i];
            float dot, denom;
            dot_and_denom(p, nr, dot, denom);
            if (!(denom <= 1e-6f)) {
                const float abs_cos = fabsf(dot / denom);
                keep = !(abs_cos < min_cos || abs_cos > max_cos);
            }
        }
        flags[i] = keep;
    }
}

template <int SRC>
__global__ __launch_bounds__(kBlock) void intensity_correct_kernel(const float4* __restrict__ points,
                                                                   const float4* __restrict__ normals,
                                                                   const float4* __restrict__ covs, float* intensities, unsigned n,
                                                                   float exponent, float scale, float min_intensity,
                                                                   float max_intensity, float ref_distance, float angle_exponent) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 p = points[i];
        const float intensity = intensities[i];
        float angle_factor = 1.0f;
        if (SRC != kNoAngle) {
            const float4 nr = SRC == kFromCovs ? normal_of(load_cov(covs + 4 * (size_t)i), p) : normals[i];
            float dot, denom;
            dot_and_denom(p, nr, dot, denom);
            if (!(denom <= 1e-6f)) angle_factor = powf(fmaxf(fabsf(dot / denom), 1e-3f), -angle_exponent);
        }
        const float dist = sqrtf(p.x * p.x + p.y * p.y + p.z * p.z);
        const float dist_factor = powf(dist / ref_distance, exponent);
        intensities[i] = fminf(fmaxf(intensity * dist_factor * angle_factor * scale, min_intensity), max_intensity);  // sycl::clamp
    }
}

// The sensor-local basis of a point (intensity_gaussian.hpp:40-62) and the running sums of its neighbourhood.
struct GaussAcc {
    float px, py, pz, rx, ry, rz, ax, ay, ex, ey, ez;
    float sum_w = 0.0f, sum_wI = 0.0f;
    // one neighbour (:66-81). An index outside [0, n) is skipped: -1 padding, or a result of another cloud.
    __device__ __forceinline__ void add(int32_t idx, const float4* __restrict__ points, const float* __restrict__ intensities,
                                        unsigned n, float inv2_az, float inv2_el, float inv2_r) {
        if ((unsigned)idx >= n) return;
        const float4 q = points[idx];
        const float iq = intensities[idx];
        const float dpx = q.x - px, dpy = q.y - py, dpz = q.z - pz;
        const float dp_r = dpx * rx + dpy * ry + dpz * rz;
        const float dp_az = dpx * ax + dpy * ay;
        const float dp_el = dpx * ex + dpy * ey + dpz * ez;
        const float exponent = dp_r * dp_r * inv2_r + dp_az * dp_az * inv2_az + dp_el * dp_el * inv2_el;
        const float w = expf(-exponent);
        sum_w += w;
        sum_wI += w * iq;
    }
};

template <bool NORMALIZE, bool ROW16>  // ROW16: k_stride % 4 == 0 and a 16-byte aligned index array
__global__ __launch_bounds__(kBlock) void intensity_gaussian_kernel(const float4* __restrict__ points,
                                                                    const float* __restrict__ intensities,
                                                                    const int32_t* __restrict__ knn, unsigned n, unsigned k_stride,
                                                                    unsigned k_use, float inv2_az, float inv2_el, float inv2_r,
                                                                    float mean_min, float* __restrict__ out) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 p = points[i];
        const float own = intensities[i];
        float mean = own;
        const float r = sqrtf(p.x * p.x + p.y * p.y + p.z * p.z);
        if (!(r < 1e-6f)) {
            GaussAcc g;
            g.px = p.x; g.py = p.y; g.pz = p.z;
            g.rx = p.x / r; g.ry = p.y / r; g.rz = p.z / r;
            const float rxy = sqrtf(p.x * p.x + p.y * p.y);
            const bool near_zenith = rxy < 1e-6f;
            const float inv_rxy = 1.0f / fmaxf(rxy, 1e-6f);
            g.ax = near_zenith ? 1.0f : (-p.y * inv_rxy);
            g.ay = near_zenith ? 0.0f : (p.x * inv_rxy);
            g.ex = near_zenith ? 0.0f : (-g.rz * g.ay);
            g.ey = near_zenith ? 1.0f : (g.rz * g.ax);
            g.ez = near_zenith ? 0.0f : (rxy / r);
            const int32_t* __restrict__ row = knn + (size_t)i * k_stride;
            if (ROW16) {
                const int4* __restrict__ row4 = reinterpret_cast<const int4*>(row);
                for (unsigned j = 0; j < k_use; j += 4) {  // (j + 3 < k_stride: the stride is a multiple of 4)
                    const int4 q = row4[j >> 2];
                    g.add(q.x, points, intensities, n, inv2_az, inv2_el, inv2_r);
                    if (j + 1 < k_use) g.add(q.y, points, intensities, n, inv2_az, inv2_el, inv2_r);
                    if (j + 2 < k_use) g.add(q.z, points, intensities, n, inv2_az, inv2_el, inv2_r);
                    if (j + 3 < k_use) g.add(q.w, points, intensities, n, inv2_az, inv2_el, inv2_r);
                }
            } else {
                for (unsigned j = 0; j < k_use; ++j) g.add(row[j], points, intensities, n, inv2_az, inv2_el, inv2_r);
            }
            mean = (g.sum_w > 0.0f) ? g.sum_wI / g.sum_w : own;
        }
        out[i] = NORMALIZE ? own / fmaxf(mean, mean_min) : mean;
    }
}

template <bool NORMALIZE>
void launch_gaussian(const float* points, const float* in, const int32_t* knn, size_t n, size_t k_stride, size_t k_use, float inv2_az,
                     float inv2_el, float inv2_r, float mean_min, float* out, hipStream_t st) {
    const float4* p4 = reinterpret_cast<const float4*>(points);
    if (k_stride % 4 == 0 && reinterpret_cast<uintptr_t>(knn) % 16 == 0)
        intensity_gaussian_kernel<NORMALIZE, true><<<stream_grid(n), kBlock, 0, st>>>(p4, in, knn, (unsigned)n, (unsigned)k_stride,
                                                                                      (unsigned)k_use, inv2_az, inv2_el, inv2_r, mean_min, out);
    else
        intensity_gaussian_kernel<NORMALIZE, false><<<stream_grid(n), kBlock, 0, st>>>(p4, in, knn, (unsigned)n, (unsigned)k_stride,
                                                                                       (unsigned)k_use, inv2_az, inv2_el, inv2_r, mean_min, out);
}

constexpr size_t kMaxPoints = (size_t)1 << 31;  // neighbour indices are int32

}  // namespace
}  // namespace sp

extern "C" int sp_angle_incidence_flags(const float* points, const float* normals, const float* covs, size_t n, float min_angle,
                                        float max_angle, uint8_t* flags_out, void* stream) {
    using namespace sp;
    if (n == 0) return SP_OK;  // (:24-25: before any check)
    if (!normals && !covs) {
        sp_set_error("[PreprocessFilter::angle_incidence_filter] Normal vector or covariance matrices must be pre-computed.");
        return SP_ERR_RUNTIME;
    }
    if (min_angle < 0.0f || max_angle > kPi * 0.5f || min_angle >= max_angle) {
        sp_set_error("[PreprocessFilter::angle_incidence_filter] Invalid angle range");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (!points || !flags_out || n >= ((size_t)1 << 32)) {
        sp_set_error("[sp_angle_incidence_flags] invalid argument (a null points / flags_out, or n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const float max_cos = std::cos(min_angle), min_cos = std::cos(max_angle);  // (:55-56, on the host)
    const float4* p4 = reinterpret_cast<const float4*>(points);
    hipStream_t st = as_stream(stream);
    if (normals)  // (:73: the normals when the cloud has them)
        angle_flags_kernel<kFromNormals><<<stream_grid(n), kBlock, 0, st>>>(p4, reinterpret_cast<const float4*>(normals), nullptr,
                                                                            (unsigned)n, min_cos, max_cos, flags_out);
    else
        angle_flags_kernel<kFromCovs><<<stream_grid(n), kBlock, 0, st>>>(p4, nullptr, reinterpret_cast<const float4*>(covs), (unsigned)n,
                                                                         min_cos, max_cos, flags_out);
    return launch_status();
}

extern "C" int sp_intensity_correct(const float* points, const float* normals, const float* covs, float* intensities, size_t n,
                                    float exponent, float scale, float min_intensity, float max_intensity, float ref_distance,
                                    float angle_exponent, void* stream) {
    using namespace sp;
    if (n == 0) return SP_OK;  // (:55-58: before any check)
    if (exponent < 0.0f) {
        sp_set_error("[correct_intensity] exponent must be non-negative");
        return SP_ERR_RUNTIME;
    }
    if (ref_distance <= 0.0f) {
        sp_set_error("[correct_intensity] ref_distance must be positive");
        return SP_ERR_RUNTIME;
    }
    if (!intensities) {
        sp_set_error("[correct_intensity] Intensity field not found");
        return SP_ERR_RUNTIME;
    }
    if (!points || n >= ((size_t)1 << 32)) {
        sp_set_error("[sp_intensity_correct] invalid argument (a null points, or n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const float4* p4 = reinterpret_cast<const float4*>(points);
    const float4* n4 = reinterpret_cast<const float4*>(normals);
    const float4* c4 = reinterpret_cast<const float4*>(covs);
    hipStream_t st = as_stream(stream);
    const bool use_angle = angle_exponent != 0.0f && (normals || covs);  // (:98)
    const unsigned grid = stream_grid(n);
    if (use_angle && normals)
        intensity_correct_kernel<kFromNormals><<<grid, kBlock, 0, st>>>(p4, n4, nullptr, intensities, (unsigned)n, exponent, scale,
                                                                        min_intensity, max_intensity, ref_distance, angle_exponent);
    else if (use_angle)
        intensity_correct_kernel<kFromCovs><<<grid, kBlock, 0, st>>>(p4, nullptr, c4, intensities, (unsigned)n, exponent, scale,
                                                                     min_intensity, max_intensity, ref_distance, angle_exponent);
    else
        intensity_correct_kernel<kNoAngle><<<grid, kBlock, 0, st>>>(p4, nullptr, nullptr, intensities, (unsigned)n, exponent, scale,
                                                                    min_intensity, max_intensity, ref_distance, angle_exponent);
    return launch_status();
}

extern "C" int sp_intensity_gaussian(const float* points, const float* intensities_in, const int32_t* knn_indices, size_t n,
                                     size_t k_stride, size_t k_use, float sigma_azimuth, float sigma_elevation, float sigma_range,
                                     float mean_min, float* intensities_out, void* stream) {
    using namespace sp;
    if (n == 0) return SP_OK;
    const bool normalize = mean_min > 0.0f;
    const char* const who = normalize ? "[intensity_local_mean_norm::normalize]" : "[intensity_gaussian::smooth_intensity]";
    char msg[160];
    if (!intensities_in) {
        snprintf(msg, sizeof msg, "%s Intensity field not found", who);
        sp_set_error(msg);
        return SP_ERR_RUNTIME;
    }
    if (k_stride < 1) {
        snprintf(msg, sizeof msg, "%s neighbors.k must be >= 1", who);
        sp_set_error(msg);
        return SP_ERR_RUNTIME;
    }
    if (sigma_azimuth <= 0.0f || sigma_elevation <= 0.0f || sigma_range <= 0.0f) {
        snprintf(msg, sizeof msg, "%s All sigma values must be positive", who);
        sp_set_error(msg);
        return SP_ERR_RUNTIME;
    }
    if (intensities_out == intensities_in) {
        sp_set_error("[sp_intensity_gaussian] intensities_out must not be intensities_in (the kernel reads the neighbours' intensities)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (!points || !knn_indices || !intensities_out || k_use < 1 || k_use > k_stride || k_stride >= ((size_t)1 << 31) ||
        n >= kMaxPoints) {
        sp_set_error("[sp_intensity_gaussian] invalid argument (a null points / knn_indices / intensities_out, k_use outside "
                     "[1, k_stride], or n >= 2^31)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    // (:112-114, on the host)
    const float inv2_az = 0.5f / (sigma_azimuth * sigma_azimuth);
    const float inv2_el = 0.5f / (sigma_elevation * sigma_elevation);
    const float inv2_r = 0.5f / (sigma_range * sigma_range);
    hipStream_t st = as_stream(stream);
    if (normalize)
        launch_gaussian<true>(points, intensities_in, knn_indices, n, k_stride, k_use, inv2_az, inv2_el, inv2_r, mean_min, intensities_out, st);
    else
        launch_gaussian<false>(points, intensities_in, knn_indices, n, k_stride, k_use, inv2_az, inv2_el, inv2_r, mean_min, intensities_out, st);
    return launch_status();
}
