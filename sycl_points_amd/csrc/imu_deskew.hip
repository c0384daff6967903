// IMU deskew for gfx950 (replaces the kernel of deskew::deskew_point_cloud_imu, algorithms/deskew/imu_deskew.hpp:330-411).
// The trajectory the kernel interpolates is built on the host (imu_preintegration.hip), one 64-byte row per interval
// [i, i + 1] of it: t_lo, t_hi, q0[4], omega[3], t0[3], t1 - t0[3], pad.
//
// The motion of sp_deskew_row.h's row body, in the reference's order: the reference's bisection over the trajectory's stamps
// (lo = 0, hi = n_traj - 1, mid = (lo + hi) / 2, stamp[mid] <= t), alpha = (t_hi > t_lo) ?
// clamp((t - t_lo) / (t_hi - t_lo), 0, 1) : 0, q = quat_mult(q0, so3_exp(omega * alpha)), R = quat_to_rot(q),
// tr = fma(t1 - t0, alpha, t0), p' = multiply<3,3>(R, p) + tr with w carried.
// omega = so3_log(conj(q0) * (+-q1)) is quat_slerp's first half (:54-73). The reference recomputes it for every point, but it is a
// function of the interval alone, so reading it from the row gives the same bits and leaves no atan2f on the device: what is
// left per point is sqrtf, sinf, cosf and a division, the functions of the constant-velocity kernel (deskew.hip).
//
// The bisection runs on the rows: stamp[k] is row[k].t_lo for k < n_intervals and row[n_intervals - 1].t_hi for the last pose.
// mid lies strictly between lo and hi, so it is in [1, n_intervals - 1] and the last pose's stamp is never compared - the
// reference does not compare it either. lo starts at 0 and only takes values of mid; hi starts at n_intervals: whatever the
// table holds (equal or unordered stamps, NaN), every row index read is in [0, n_intervals - 1].
//
// A workgroup stages the rows in LDS, and their t_lo once more as a dense array (the bisection's reads then hit 64 banks
// instead of the 4 a 64-byte stride would), when there are at most kLdsRows = 300 of them: 300 * 68 B = 20 400 B per
// workgroup, so the eight 256-lane workgroups that fill a CU's 32 wave slots take 163 200 B of its 163 840 B and the staging
// never costs occupancy. A 200 Hz to 1 kHz IMU gives 25 to 250 rows per 0.1 s scan. Longer tables are read from global memory
// (they stay in L2: 5000 rows are 320 KB).
#include <cmath>

#include "sp_deskew_row.h"
#include "sp_math.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr unsigned kLdsRows = 300;

// quat_mult (imu_deskew.hpp:43-50), the fma chains as written
__device__ __forceinline__ void quat_mult(const float a[4], const float b[4], float r[4]) {
    r[0] = fmaf(a[3], b[0], fmaf(+a[0], b[3], fmaf(+a[1], b[2], -a[2] * b[1])));
    r[1] = fmaf(a[3], b[1], fmaf(-a[0], b[2], fmaf(+a[1], b[3], +a[2] * b[0])));
    r[2] = fmaf(a[3], b[2], fmaf(+a[0], b[1], fmaf(-a[1], b[0], +a[2] * b[3])));
    r[3] = fmaf(a[3], b[3], fmaf(-a[0], b[0], fmaf(-a[1], b[1], -a[2] * b[2])));
}

// rows: the interval table (4 float4 per row); stamps[k * STAMP_STRIDE] = row[k].t_lo
template <int STAMP_STRIDE>
struct ImuTrajectory {
    const float4* rows;
    const float* stamps;
    unsigned n_intervals;
    __device__ __forceinline__ float4 operator()(float ts, const float4 p, float R[3][3]) const {
        unsigned lo = 0, hi = n_intervals;  // hi = n_traj - 1
        while (hi - lo > 1) {
            const unsigned mid = (lo + hi) / 2;
            if (stamps[(size_t)mid * STAMP_STRIDE] <= ts)
                lo = mid;
            else
                hi = mid;
        }
        const float4 r0 = rows[4 * (size_t)lo + 0], r1 = rows[4 * (size_t)lo + 1], r2 = rows[4 * (size_t)lo + 2],
                     r3 = rows[4 * (size_t)lo + 3];
        const float t_lo = r0.x, t_hi = r0.y;
        float alpha = 0.0f;
        if (t_hi > t_lo) alpha = fminf(fmaxf((ts - t_lo) / (t_hi - t_lo), 0.0f), 1.0f);  // sycl::clamp
        const float q0[4] = {r0.z, r0.w, r1.x, r1.y};
        const float wa[3] = {r1.z * alpha, r1.w * alpha, r2.x * alpha};
        float dq[4], q[4];
        so3_exp(wa, dq);
        quat_mult(q0, dq, q);
        quat_to_rot(q, R);
        const float tx = fmaf(r3.x, alpha, r2.y), ty = fmaf(r3.y, alpha, r2.z), tz = fmaf(r3.z, alpha, r2.w);
        return make_float4(chain3(R[0][0], p.x, R[0][1], p.y, R[0][2], p.z) + tx, chain3(R[1][0], p.x, R[1][1], p.y, R[1][2], p.z) + ty,
                           chain3(R[2][0], p.x, R[2][1], p.y, R[2][2], p.z) + tz, p.w);
    }
};

// lds_rows: n_intervals when the launch carries n_intervals * 68 bytes of dynamic LDS, else 0 (the rows are read where they are)
template <bool COVS, bool NORMALS>
__global__ __launch_bounds__(kBlock) void imu_deskew_kernel(const float4* points, const float4* covs, const float4* normals,
                                                            const float* __restrict__ t_ms, unsigned n,
                                                            const float4* __restrict__ intervals, unsigned n_intervals,
                                                            unsigned lds_rows, float4* points_out, float4* covs_out,
                                                            float4* normals_out) {
    extern __shared__ float4 s_rows[];  // 4 * lds_rows float4, then lds_rows floats
    if (lds_rows != 0u) {
        float* s_stamps = reinterpret_cast<float*>(s_rows + 4 * (size_t)lds_rows);
        for (unsigned k = threadIdx.x; k < 4 * lds_rows; k += kBlock) s_rows[k] = intervals[k];
        for (unsigned k = threadIdx.x; k < lds_rows; k += kBlock) s_stamps[k] = intervals[4 * (size_t)k].x;
        __syncthreads();
        deskew_rows<COVS, NORMALS>(points, covs, normals, t_ms, n, ImuTrajectory<1>{s_rows, s_stamps, n_intervals}, points_out,
                                   covs_out, normals_out);
    } else {
        deskew_rows<COVS, NORMALS>(points, covs, normals, t_ms, n,
                                   ImuTrajectory<16>{intervals, reinterpret_cast<const float*>(intervals), n_intervals}, points_out,
                                   covs_out, normals_out);
    }
}

}  // namespace
}  // namespace sp

extern "C" int sp_deskew_imu(const float* points, const float* covs, const float* normals, const float* timestamp_offsets_ms,
                             size_t n, const float* intervals, size_t n_intervals, float* points_out, float* covs_out,
                             float* normals_out, void* stream) {
    using namespace sp;
    if (!deskew_cloud_args_ok(points, covs, normals, timestamp_offsets_ms, n, points_out, covs_out, normals_out) || !intervals ||
        n_intervals < 1 || n_intervals >= ((size_t)1 << 31)) {
        sp_set_error("[sp_deskew_imu] invalid argument (a null points / timestamp_offsets_ms / points_out / intervals, covs or "
                     "normals given without their output or the other way round, n_intervals < 1 or >= 2^31, or n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return SP_OK;
    const unsigned lds_rows = n_intervals <= kLdsRows ? (unsigned)n_intervals : 0u;
    deskew_dispatch(covs != nullptr, normals != nullptr, [&](auto C, auto N) {
        imu_deskew_kernel<C.value, N.value><<<stream_grid(n), kBlock, (size_t)lds_rows * 68, as_stream(stream)>>>(
            as_float4(points), as_float4(covs), as_float4(normals), timestamp_offsets_ms, (unsigned)n, as_float4(intervals),
            (unsigned)n_intervals, lds_rows, as_float4(points_out), as_float4(covs_out), as_float4(normals_out));
    });
    return launch_status();
}
