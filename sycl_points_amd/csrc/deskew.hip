// Constant-velocity deskew for gfx950 (replaces the kernel of deskew::deskew_point_cloud_constant_velocity,
// algorithms/deskew/relative_pose_deskew.hpp:120-172) and the host-side relative twist that feeds it (:103-104).
//
// Per point, in the reference's order: ts = t_ms * 1e-3f; a non-finite ts copies the row; otherwise
// tau = clamp(ts / duration, 0, 1), a = twist * tau, M = se3_exp(a), p' = multiply<4,4>(M, p),
// R = quaternion_to_rotation_matrix(so3_exp(a[0..2])) (the rotation block of M: the same function of the same
// argument), n' = (R n, 0), C' = R (C3 R^T) in the top-left 3x3 of a zeroed 4x4. se3_exp / so3_exp / quat_to_rot and
// the fma chains are sp_math.h's, unchanged.
//
// One lane per point, no LDS, no cross-lane work; the twist and the duration are kernel arguments (uniform: SGPRs).
// Every access is 16 bytes wide except the 4-byte time stamp. One instantiation per attribute set:
//   points                 16 + 4 + 16              =  36 B/pt
//   points + normals       36 + 16 + 16             =  68 B/pt
//   points + covs          36 + 48 + 64             = 148 B/pt   (the input covariance's first three columns only)
//   points + covs + normals                         = 180 B/pt   (a non-finite row reads the fourth column too: 196)
// Every lane reads its whole row before it stores anything, so *_out == *_in is legal. That is a deliberate deviation:
// the reference zeroes covs_out[idx] / normals_out[idx] before it reads the inputs (:160-166), so its in-place call
// returns zero normals and covariances; here in-place returns the rotated ones.
#include <cmath>

#include "sp_common.h"
#include "sp_math.h"
#include "sp_pose_math.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

struct Twist6 {  // by value in the kernarg segment
    float v[6];
};

template <bool COVS, bool NORMALS>
__global__ __launch_bounds__(kBlock) void deskew_kernel(const float4* points, const float4* covs, const float4* normals,
                                                        const float* __restrict__ t_ms, unsigned n, Twist6 twist,
                                                        float duration, float4* points_out, float4* covs_out,
                                                        float4* normals_out) {
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
        const float tau = fminf(fmaxf(ts / duration, 0.0f), 1.0f);  // sycl::clamp
        float a[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = twist.v[k] * tau;
        const Rigid M = se3_exp(a);
        // multiply<4,4>(M, p): per row fma(M(i,3), w, fma(M(i,2), z, fma(M(i,1), y, fma(M(i,0), x, 0)))); row 3 is 0 0 0 1
        float4 q;
        q.x = fmaf(M.t[0], p.w, chain3(M.R[0][0], p.x, M.R[0][1], p.y, M.R[0][2], p.z));
        q.y = fmaf(M.t[1], p.w, chain3(M.R[1][0], p.x, M.R[1][1], p.y, M.R[1][2], p.z));
        q.z = fmaf(M.t[2], p.w, chain3(M.R[2][0], p.x, M.R[2][1], p.y, M.R[2][2], p.z));
        q.w = fmaf(1.0f, p.w, chain3(0.0f, p.x, 0.0f, p.y, 0.0f, p.z));
        points_out[i] = q;
        if (NORMALS)
            normals_out[i] = make_float4(chain3(M.R[0][0], nr.x, M.R[0][1], nr.y, M.R[0][2], nr.z),
                                         chain3(M.R[1][0], nr.x, M.R[1][1], nr.y, M.R[1][2], nr.z),
                                         chain3(M.R[2][0], nr.x, M.R[2][1], nr.y, M.R[2][2], nr.z), 0.0f);
        if (COVS) {
            Mat3 C, R;  // column-major storage: C(i, k) is component i of column k
            C.m[0][0] = c0.x; C.m[1][0] = c0.y; C.m[2][0] = c0.z;
            C.m[0][1] = c1.x; C.m[1][1] = c1.y; C.m[2][1] = c1.z;
            C.m[0][2] = c2.x; C.m[1][2] = c2.y; C.m[2][2] = c2.z;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) R.m[r][c] = M.R[r][c];
            const Mat3 O = matmul(R, matmul_bt(C, R));  // R (C R^T), the inner product first
            covs_out[4 * (size_t)i + 0] = make_float4(O.m[0][0], O.m[1][0], O.m[2][0], 0.0f);
            covs_out[4 * (size_t)i + 1] = make_float4(O.m[0][1], O.m[1][1], O.m[2][1], 0.0f);
            covs_out[4 * (size_t)i + 2] = make_float4(O.m[0][2], O.m[1][2], O.m[2][2], 0.0f);
            covs_out[4 * (size_t)i + 3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

template <bool COVS, bool NORMALS>
void launch_deskew(const float* points, const float* covs, const float* normals, const float* t_ms, size_t n, const Twist6& twist,
                   float duration, float* points_out, float* covs_out, float* normals_out, hipStream_t st) {
    deskew_kernel<COVS, NORMALS><<<stream_grid(n), kBlock, 0, st>>>(
        reinterpret_cast<const float4*>(points), reinterpret_cast<const float4*>(covs), reinterpret_cast<const float4*>(normals),
        t_ms, (unsigned)n, twist, duration, reinterpret_cast<float4*>(points_out), reinterpret_cast<float4*>(covs_out),
        reinterpret_cast<float4*>(normals_out));
}

}  // namespace
}  // namespace sp

extern "C" int sp_deskew_constant_velocity(const float* points, const float* covs, const float* normals,
                                           const float* timestamp_offsets_ms, size_t n, const float* delta_twist6_host,
                                           float scan_duration_seconds, float* points_out, float* covs_out, float* normals_out,
                                           void* stream) {
    using namespace sp;
    if (!points || !timestamp_offsets_ms || !points_out || !delta_twist6_host || (covs == nullptr) != (covs_out == nullptr) ||
        (normals == nullptr) != (normals_out == nullptr) || !(scan_duration_seconds > 0.0f) ||
        !(scan_duration_seconds <= FLT_MAX) || n >= ((size_t)1 << 32)) {
        sp_set_error("[sp_deskew_constant_velocity] invalid argument (a null points / timestamp_offsets_ms / points_out / twist, "
                     "covs or normals given without their output or the other way round, a duration that is not positive and "
                     "finite, or n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return SP_OK;
    Twist6 twist;
    for (int k = 0; k < 6; ++k) twist.v[k] = delta_twist6_host[k];
    hipStream_t st = as_stream(stream);
    if (covs && normals)
        launch_deskew<true, true>(points, covs, normals, timestamp_offsets_ms, n, twist, scan_duration_seconds, points_out, covs_out, normals_out, st);
    else if (covs)
        launch_deskew<true, false>(points, covs, normals, timestamp_offsets_ms, n, twist, scan_duration_seconds, points_out, covs_out, normals_out, st);
    else if (normals)
        launch_deskew<false, true>(points, covs, normals, timestamp_offsets_ms, n, twist, scan_duration_seconds, points_out, covs_out, normals_out, st);
    else
        launch_deskew<false, false>(points, covs, normals, timestamp_offsets_ms, n, twist, scan_duration_seconds, points_out, covs_out, normals_out, st);
    return launch_status();
}

extern "C" void sp_relative_twist_host(const float* prev_pose16, const float* cur_pose16, float* twist6_out) {
    sp::se3_log(sp::rigid_mul(sp::rigid_inverse(sp::load_rigid_colmajor(prev_pose16)), sp::load_rigid_colmajor(cur_pose16)), twist6_out);
}
