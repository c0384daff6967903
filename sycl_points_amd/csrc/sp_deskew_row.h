// The row body of the deskew kernels (deskew.hip: constant velocity; imu_deskew.hip: an IMU trajectory) and the host side they
// share. A motion model is a functor `float4 operator()(float ts, float4 p, float R[3][3]) const`: the time stamp in seconds and
// the point in, the rotation at that time and the moved point out; a kernel builds it from its own arguments and hands it over
// by value. Everything else is here, once.
//
// One lane per point, grid-stride, no cross-lane work. Per row: ts = t_ms * 1e-3f; a non-finite ts copies the row; otherwise
// p' = motion(ts, p, R), n' = (R n, 0), C' = R (C3 R^T) in the top-left 3x3 of a zeroed 4x4 (the chain3 fma chains of sp_math.h).
// Read order: stamp, point, normal, covariance columns 0-2, all before the branch; the fourth column only in a copied row.
// Every access is 16 bytes wide except the 4-byte time stamp. One instantiation per attribute set:
//   points                 16 + 4 + 16              =  36 B/pt
//   points + normals       36 + 16 + 16             =  68 B/pt
//   points + covs          36 + 48 + 64             = 148 B/pt   (the input covariance's first three columns only)
//   points + covs + normals                         = 180 B/pt   (a non-finite row reads the fourth column too: 196)
// Aliasing: every lane reads its whole row before it stores anything, so *_out == *_in is legal, and no cloud pointer here may
// be __restrict__. That is a deliberate deviation: the reference zeroes covs_out[idx] / normals_out[idx] before it reads the
// inputs (relative_pose_deskew.hpp:160-166, imu_deskew.hpp:398, :403), so its in-place call returns zero normals and
// covariances; here in-place returns the rotated ones.
#pragma once
#include <type_traits>

#include "sp_common.h"
#include "sp_cov_normal.h"

namespace sp {

template <bool COVS, bool NORMALS, class Motion>
__device__ __forceinline__ void deskew_rows(const float4* points, const float4* covs, const float4* normals,
                                            const float* __restrict__ t_ms, unsigned n, const Motion motion, float4* points_out,
                                            float4* covs_out, float4* normals_out) {
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        // the whole row first (the outputs may be the inputs)
        const float ts = t_ms[i] * 1e-3f;
        const float4 p = points[i];
        float4 nr = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c0 = nr, c1 = nr, c2 = nr;
        if (NORMALS) nr = normals[i];
        if (COVS) {
            c0 = covs[4 * (size_t)i + 0];
            c1 = covs[4 * (size_t)i + 1];
            c2 = covs[4 * (size_t)i + 2];
        }
        if (!(fabsf(ts) <= FLT_MAX)) {  // !isfinite: the row as it is, all 16 floats of the covariance
            float4 c3 = nr;
            if (COVS) c3 = covs[4 * (size_t)i + 3];
            points_out[i] = p;
            if (NORMALS) normals_out[i] = nr;
            if (COVS) {
                covs_out[4 * (size_t)i + 0] = c0;
                covs_out[4 * (size_t)i + 1] = c1;
                covs_out[4 * (size_t)i + 2] = c2;
                covs_out[4 * (size_t)i + 3] = c3;
            }
            continue;
        }
        Mat3 R;
        points_out[i] = motion(ts, p, R.m);
        if (NORMALS)
            normals_out[i] = make_float4(chain3(R.m[0][0], nr.x, R.m[0][1], nr.y, R.m[0][2], nr.z),
                                         chain3(R.m[1][0], nr.x, R.m[1][1], nr.y, R.m[1][2], nr.z),
                                         chain3(R.m[2][0], nr.x, R.m[2][1], nr.y, R.m[2][2], nr.z), 0.0f);
        if (COVS) {
            // R (C R^T), the inner product first. The stores are written out: store_cov's pointer is __restrict__, and with it
            // the compiler orders the kernels' instructions differently.
            const Mat3 O = matmul(R, matmul_bt(cov_of_columns(c0, c1, c2), R));
            covs_out[4 * (size_t)i + 0] = make_float4(O.m[0][0], O.m[1][0], O.m[2][0], 0.0f);
            covs_out[4 * (size_t)i + 1] = make_float4(O.m[0][1], O.m[1][1], O.m[2][1], 0.0f);
            covs_out[4 * (size_t)i + 2] = make_float4(O.m[0][2], O.m[1][2], O.m[2][2], 0.0f);
            covs_out[4 * (size_t)i + 3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host side
inline const float4* as_float4(const float* p) { return reinterpret_cast<const float4*>(p); }
inline float4* as_float4(float* p) { return reinterpret_cast<float4*>(p); }

// What both C entries require of the cloud: points, stamps and an output; an attribute exactly when its output; n < 2^32.
inline bool deskew_cloud_args_ok(const float* points, const float* covs, const float* normals, const float* t_ms, size_t n,
                                 const float* points_out, const float* covs_out, const float* normals_out) {
    return points && t_ms && points_out && (covs == nullptr) == (covs_out == nullptr) &&
           (normals == nullptr) == (normals_out == nullptr) && n < ((size_t)1 << 32);
}

// launch(covs_tag, normals_tag) with the attribute set as compile-time constants: launch is a generic lambda that
// instantiates its kernel with <covs_tag.value, normals_tag.value>
template <class Launch>
void deskew_dispatch(bool covs, bool normals, Launch&& launch) {
    if (covs && normals)
        launch(std::true_type{}, std::true_type{});
    else if (covs)
        launch(std::true_type{}, std::false_type{});
    else if (normals)
        launch(std::false_type{}, std::true_type{});
    else
        launch(std::false_type{}, std::false_type{});
}

}  // namespace sp
