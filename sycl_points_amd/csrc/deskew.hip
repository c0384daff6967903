// Constant-velocity deskew for gfx950 (replaces the kernel of deskew::deskew_point_cloud_constant_velocity,
// algorithms/deskew/relative_pose_deskew.hpp:120-172) and the host-side relative twist that feeds it (:103-104).
//
// The motion of sp_deskew_row.h's row body, in the reference's order: tau = clamp(ts / duration, 0, 1), a = twist * tau,
// M = se3_exp(a), p' = multiply<4,4>(M, p), R = quaternion_to_rotation_matrix(so3_exp(a[0..2])) (the rotation block of M: the
// same function of the same argument). se3_exp / so3_exp / quat_to_rot and the fma chains are sp_math.h's, unchanged.
// No LDS; the twist and the duration are kernel arguments (uniform: SGPRs).
#include <cmath>

#include "sp_deskew_row.h"
#include "sp_math.h"
#include "sp_pose_math.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

struct Twist6 {  // by value in the kernarg segment
    float v[6];
};

struct ConstantVelocity {
    Twist6 twist;
    float duration;
    __device__ __forceinline__ float4 operator()(float ts, const float4 p, float R[3][3]) const {
        const float tau = fminf(fmaxf(ts / duration, 0.0f), 1.0f);  // sycl::clamp
        float a[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = twist.v[k] * tau;
        const Rigid M = se3_exp(a);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[r][c] = M.R[r][c];
        // multiply<4,4>(M, p): per row fma(M(i,3), w, fma(M(i,2), z, fma(M(i,1), y, fma(M(i,0), x, 0)))); row 3 is 0 0 0 1, and
        // its chain stays: an infinite coordinate makes w NaN
        return make_float4(fmaf(M.t[0], p.w, chain3(M.R[0][0], p.x, M.R[0][1], p.y, M.R[0][2], p.z)),
                           fmaf(M.t[1], p.w, chain3(M.R[1][0], p.x, M.R[1][1], p.y, M.R[1][2], p.z)),
                           fmaf(M.t[2], p.w, chain3(M.R[2][0], p.x, M.R[2][1], p.y, M.R[2][2], p.z)),
                           fmaf(1.0f, p.w, chain3(0.0f, p.x, 0.0f, p.y, 0.0f, p.z)));
    }
};

template <bool COVS, bool NORMALS>
__global__ __launch_bounds__(kBlock) void deskew_kernel(const float4* points, const float4* covs, const float4* normals,
                                                        const float* __restrict__ t_ms, unsigned n, Twist6 twist,
                                                        float duration, float4* points_out, float4* covs_out,
                                                        float4* normals_out) {
    deskew_rows<COVS, NORMALS>(points, covs, normals, t_ms, n, ConstantVelocity{twist, duration}, points_out, covs_out, normals_out);
}

}  // namespace
}  // namespace sp

extern "C" int sp_deskew_constant_velocity(const float* points, const float* covs, const float* normals,
                                           const float* timestamp_offsets_ms, size_t n, const float* delta_twist6_host,
                                           float scan_duration_seconds, float* points_out, float* covs_out, float* normals_out,
                                           void* stream) {
    using namespace sp;
    if (!deskew_cloud_args_ok(points, covs, normals, timestamp_offsets_ms, n, points_out, covs_out, normals_out) ||
        !delta_twist6_host || !(scan_duration_seconds > 0.0f) || !(scan_duration_seconds <= FLT_MAX)) {
        sp_set_error("[sp_deskew_constant_velocity] invalid argument (a null points / timestamp_offsets_ms / points_out / twist, "
                     "covs or normals given without their output or the other way round, a duration that is not positive and "
                     "finite, or n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return SP_OK;
    Twist6 twist;
    for (int k = 0; k < 6; ++k) twist.v[k] = delta_twist6_host[k];
    deskew_dispatch(covs != nullptr, normals != nullptr, [&](auto C, auto N) {
        deskew_kernel<C.value, N.value><<<stream_grid(n), kBlock, 0, as_stream(stream)>>>(
            as_float4(points), as_float4(covs), as_float4(normals), timestamp_offsets_ms, (unsigned)n, twist, scan_duration_seconds,
            as_float4(points_out), as_float4(covs_out), as_float4(normals_out));
    });
    return launch_status();
}

extern "C" void sp_relative_twist_host(const float* prev_pose16, const float* cur_pose16, float* twist6_out) {
    sp::se3_log(sp::rigid_mul(sp::rigid_inverse(sp::load_rigid_colmajor(prev_pose16)), sp::load_rigid_colmajor(cur_pose16)), twist6_out);
}
