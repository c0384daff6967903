// IMU deskew for gfx950 (replaces the kernel of deskew::deskew_point_cloud_imu, algorithms/deskew/imu_deskew.hpp:330-411).
// The trajectory the kernel interpolates is built on the host (imu_preintegration.hip), one 64-byte row per interval
// [i, i + 1] of it: t_lo, t_hi, q0[4], omega[3], t0[3], t1 - t0[3], pad.
//
// Per point, in the reference's order: t = t_ms * 1e-3f; a non-finite t copies the row; otherwise the reference's bisection
// over the trajectory's stamps (lo = 0, hi = n_traj - 1, mid = (lo + hi) / 2, stamp[mid] <= t), alpha = (t_hi > t_lo) ?
// clamp((t - t_lo) / (t_hi - t_lo), 0, 1) : 0, q = quat_mult(q0, so3_exp(omega * alpha)), R = quat_to_rot(q),
// tr = fma(t1 - t0, alpha, t0), p' = multiply<3,3>(R, p) + tr with w carried, n' = (R n, 0), C' = R (C3 R^T) in a zeroed 4x4.
// omega = so3_log(conj(q0) * (+-q1)) is quat_slerp's first half (:54-73). The reference recomputes it for every point, but it is a
// function of the interval alone, so reading it from the row gives the same bits and leaves no atan2f on the device: what is
// left per point is sqrtf, sinf, cosf and a division, the functions of the constant-velocity kernel (deskew.hip).
//
// The bisection runs on the rows: stamp[k] is row[k].t_lo for k < n_intervals and row[n_intervals - 1].t_hi for the last pose.
// mid lies strictly between lo and hi, so it is in [1, n_intervals - 1] and the last pose's stamp is never compared - the
// reference does not compare it either. lo starts at 0 and only takes values of mid; hi starts at n_intervals: whatever the
// table holds (equal or unordered stamps, NaN), every row index read is in [0, n_intervals - 1].
//
// One lane per point, grid-stride. A workgroup stages the rows in LDS, and their t_lo once more as a dense array (the
// bisection's reads then hit 64 banks instead of the 4 a 64-byte stride would), when there are at most kLdsRows = 300 of
// them: 300 * 68 B = 20 400 B per workgroup, so the eight 256-lane workgroups that fill a CU's 32 wave slots take 163 200 B
// of its 163 840 B and the staging never costs occupancy. A 200 Hz to 1 kHz IMU gives 25 to 250 rows per 0.1 s scan. Longer
// tables are read from global memory (they stay in L2: 5000 rows are 320 KB). Every access to the cloud is 16 bytes wide
// except the 4-byte time stamp; bytes per point as in deskew.hip (36 / 68 / 148 / 180). Every lane reads its whole row
// before it stores anything, so *_out == *_in is legal - the deviation deskew.hip documents: the reference zeroes
// covs_out[idx] / normals_out[idx] before it reads the inputs (:398, :403), so its in-place call returns zeros there.
#include <cmath>

#include "sp_common.h"
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
template <bool COVS, bool NORMALS, int STAMP_STRIDE>
__device__ __forceinline__ void deskew_points(const float4* points, const float4* covs, const float4* normals,
                                              const float* __restrict__ t_ms, unsigned n, const float4* rows, const float* stamps,
                                              unsigned n_intervals, float4* points_out, float4* covs_out, float4* normals_out) {
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
        float dq[4], q[4], R[3][3];
        so3_exp(wa, dq);
        quat_mult(q0, dq, q);
        quat_to_rot(q, R);
        const float tx = fmaf(r3.x, alpha, r2.y), ty = fmaf(r3.y, alpha, r2.z), tz = fmaf(r3.z, alpha, r2.w);
        points_out[i] = make_float4(chain3(R[0][0], p.x, R[0][1], p.y, R[0][2], p.z) + tx,
                                    chain3(R[1][0], p.x, R[1][1], p.y, R[1][2], p.z) + ty,
                                    chain3(R[2][0], p.x, R[2][1], p.y, R[2][2], p.z) + tz, p.w);
        if (NORMALS)
            normals_out[i] = make_float4(chain3(R[0][0], nr.x, R[0][1], nr.y, R[0][2], nr.z),
                                         chain3(R[1][0], nr.x, R[1][1], nr.y, R[1][2], nr.z),
                                         chain3(R[2][0], nr.x, R[2][1], nr.y, R[2][2], nr.z), 0.0f);
        if (COVS) {
            Mat3 C, Rm;  // C(i, k) is component i of column k
            C.m[0][0] = c0.x; C.m[1][0] = c0.y; C.m[2][0] = c0.z;
            C.m[0][1] = c1.x; C.m[1][1] = c1.y; C.m[2][1] = c1.z;
            C.m[0][2] = c2.x; C.m[1][2] = c2.y; C.m[2][2] = c2.z;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Rm.m[r][c] = R[r][c];
            const Mat3 O = matmul(Rm, matmul_bt(C, Rm));  // R (C R^T), the inner product first
            covs_out[4 * (size_t)i + 0] = make_float4(O.m[0][0], O.m[1][0], O.m[2][0], 0.0f);
            covs_out[4 * (size_t)i + 1] = make_float4(O.m[0][1], O.m[1][1], O.m[2][1], 0.0f);
            covs_out[4 * (size_t)i + 2] = make_float4(O.m[0][2], O.m[1][2], O.m[2][2], 0.0f);
            covs_out[4 * (size_t)i + 3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

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
        deskew_points<COVS, NORMALS, 1>(points, covs, normals, t_ms, n, s_rows, s_stamps, n_intervals, points_out, covs_out,
                                        normals_out);
    } else {
        deskew_points<COVS, NORMALS, 16>(points, covs, normals, t_ms, n, intervals, reinterpret_cast<const float*>(intervals),
                                         n_intervals, points_out, covs_out, normals_out);
    }
}

template <bool COVS, bool NORMALS>
void launch_imu_deskew(const float* points, const float* covs, const float* normals, const float* t_ms, size_t n,
                       const float* intervals, size_t n_intervals, float* points_out, float* covs_out, float* normals_out,
                       hipStream_t st) {
    const unsigned lds_rows = n_intervals <= kLdsRows ? (unsigned)n_intervals : 0u;
    imu_deskew_kernel<COVS, NORMALS><<<stream_grid(n), kBlock, (size_t)lds_rows * 68, st>>>(
        reinterpret_cast<const float4*>(points), reinterpret_cast<const float4*>(covs), reinterpret_cast<const float4*>(normals),
        t_ms, (unsigned)n, reinterpret_cast<const float4*>(intervals), (unsigned)n_intervals, lds_rows,
        reinterpret_cast<float4*>(points_out), reinterpret_cast<float4*>(covs_out), reinterpret_cast<float4*>(normals_out));
}

}  // namespace
}  // namespace sp

extern "C" int sp_deskew_imu(const float* points, const float* covs, const float* normals, const float* timestamp_offsets_ms,
                             size_t n, const float* intervals, size_t n_intervals, float* points_out, float* covs_out,
                             float* normals_out, void* stream) {
    using namespace sp;
    if (!points || !timestamp_offsets_ms || !points_out || !intervals || (covs == nullptr) != (covs_out == nullptr) ||
        (normals == nullptr) != (normals_out == nullptr) || n_intervals < 1 || n_intervals >= ((size_t)1 << 31) ||
        n >= ((size_t)1 << 32)) {
        sp_set_error("[sp_deskew_imu] invalid argument (a null points / timestamp_offsets_ms / points_out / intervals, covs or "
                     "normals given without their output or the other way round, n_intervals < 1 or >= 2^31, or n >= 2^32)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return SP_OK;
    hipStream_t st = as_stream(stream);
    if (covs && normals)
        launch_imu_deskew<true, true>(points, covs, normals, timestamp_offsets_ms, n, intervals, n_intervals, points_out, covs_out, normals_out, st);
    else if (covs)
        launch_imu_deskew<true, false>(points, covs, normals, timestamp_offsets_ms, n, intervals, n_intervals, points_out, covs_out, normals_out, st);
    else if (normals)
        launch_imu_deskew<false, true>(points, covs, normals, timestamp_offsets_ms, n, intervals, n_intervals, points_out, covs_out, normals_out, st);
    else
        launch_imu_deskew<false, false>(points, covs, normals, timestamp_offsets_ms, n, intervals, n_intervals, points_out, covs_out, normals_out, st);
    return launch_status();
}
