// CPU restatement of the IMU deskew kernel (deskew/imu_deskew.hpp:330-411 with detail::quat_mult, quat_slerp and
// interpolate_trajectory_pose, :43-89): float32 in the reference's order with the explicit fmaf chains of eigen_utils.hpp
// (oracle/oracle_math.hpp), the slerp evaluated PER POINT exactly as written - not hoisted to the interval as the library does -
// and a float64 evaluation of the same formula as the yardstick of both. Built by the tests with g++ -O2 -ffp-contract=off as a
// shared library. The trajectory is the reference's: 8 floats per pose (q xyzw, t xyz, stamp).
//
// Unlike the reference, both read a row completely before they write it, so the outputs may be the inputs (the library's
// documented deviation: the reference zeroes normals_out / covs_out first and returns zeros in place).
#include <cmath>
#include <cstdint>

#include "../../oracle/oracle_math.hpp"

using namespace oracle;

namespace {

Vec4 quat_mult(const Vec4& a, const Vec4& b) {  // :43-50
    Vec4 r;
    r[0] = std::fmaf(a[3], b[0], std::fmaf(+a[0], b[3], std::fmaf(+a[1], b[2], -a[2] * b[1])));
    r[1] = std::fmaf(a[3], b[1], std::fmaf(-a[0], b[2], std::fmaf(+a[1], b[3], +a[2] * b[0])));
    r[2] = std::fmaf(a[3], b[2], std::fmaf(+a[0], b[1], std::fmaf(-a[1], b[0], +a[2] * b[3])));
    r[3] = std::fmaf(a[3], b[3], std::fmaf(-a[0], b[0], std::fmaf(-a[1], b[1], -a[2] * b[2])));
    return r;
}

// quat_slerp's first half (:54-73): q1 on the shorter arc, then so3_log(conj(q0) * q1)
void slerp_parts(const Vec4& q0, const Vec4& q1, Vec4& q1_signed, Vec3& omega) {
    q1_signed = q1;
    if (dot<4>(q0, q1_signed) < 0.0f) {
        q1_signed[0] *= -1.0f; q1_signed[1] *= -1.0f; q1_signed[2] *= -1.0f; q1_signed[3] *= -1.0f;
    }
    Vec4 q0_conj;
    q0_conj[0] = -q0[0]; q0_conj[1] = -q0[1]; q0_conj[2] = -q0[2]; q0_conj[3] = q0[3];
    omega = so3_log(quat_mult(q0_conj, q1_signed));
}

Vec4 quat_slerp(const Vec4& q0, const Vec4& q1, float alpha) {
    Vec4 q1_signed;
    Vec3 omega;
    slerp_parts(q0, q1, q1_signed, omega);
    return quat_mult(q0, so3_exp(scale<3, 1>(omega, alpha)));
}

// the reference's bisection (:365-373) on the trajectory's stamps
void bisect(const float* traj, uint64_t n_traj, float t_sec, uint64_t& lo, uint64_t& hi) {
    lo = 0;
    hi = n_traj - 1;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (traj[8 * mid + 7] <= t_sec)
            lo = mid;
        else
            hi = mid;
    }
}

}  // namespace

extern "C" void imu_deskew_restate(const float* points, const float* covs, const float* normals, const float* t_ms, uint64_t n,
                                   const float* traj, uint64_t n_traj, float* points_out, float* covs_out, float* normals_out) {
    for (uint64_t i = 0; i < n; ++i) {
        Vec4 p, nr;
        Mat4 C;
        for (int k = 0; k < 4; ++k) p[k] = points[4 * i + k];
        if (normals) for (int k = 0; k < 4; ++k) nr[k] = normals[4 * i + k];
        if (covs) for (int k = 0; k < 16; ++k) C[k] = covs[16 * i + k];
        const float t_sec = t_ms[i] * 1e-3f;
        if (!std::isfinite(t_sec)) {
            for (int k = 0; k < 4; ++k) points_out[4 * i + k] = p[k];
            if (normals) for (int k = 0; k < 4; ++k) normals_out[4 * i + k] = nr[k];
            if (covs) for (int k = 0; k < 16; ++k) covs_out[16 * i + k] = C[k];
            continue;
        }
        uint64_t lo, hi;
        bisect(traj, n_traj, t_sec, lo, hi);
        const float *e0 = traj + 8 * lo, *e1 = traj + 8 * hi;
        const float t_lo = e0[7], t_hi = e1[7];
        float alpha = 0.0f;
        if (t_hi > t_lo) alpha = std::fmin(std::fmax((t_sec - t_lo) / (t_hi - t_lo), 0.0f), 1.0f);  // sycl::clamp
        Vec4 q0, q1;
        for (int k = 0; k < 4; ++k) { q0[k] = e0[k]; q1[k] = e1[k]; }
        const Mat3 R = quaternion_to_rotation_matrix(quat_slerp(q0, q1, alpha));
        Vec3 t_interp, p3;
        for (int k = 0; k < 3; ++k) {
            t_interp[k] = std::fmaf(e1[4 + k] - e0[4 + k], alpha, e0[4 + k]);
            p3[k] = p[k];
        }
        const Vec3 Rp = matvec<3, 3>(R, p3);
        for (int k = 0; k < 3; ++k) points_out[4 * i + k] = Rp[k] + t_interp[k];
        points_out[4 * i + 3] = p[3];
        if (normals) {
            Vec3 n3;
            for (int k = 0; k < 3; ++k) n3[k] = nr[k];
            const Vec3 rn = matvec<3, 3>(R, n3);
            for (int k = 0; k < 3; ++k) normals_out[4 * i + k] = rn[k];
            normals_out[4 * i + 3] = 0.0f;
        }
        if (covs) {
            Mat3 C3;
            for (int c = 0; c < 3; ++c)
                for (int r = 0; r < 3; ++r) C3(r, c) = C(r, c);
            const Mat3 out = matmul<3, 3, 3>(R, matmul<3, 3, 3>(C3, transpose<3, 3>(R)));
            for (int k = 0; k < 16; ++k) covs_out[16 * i + k] = 0.0f;
            for (int c = 0; c < 3; ++c)
                for (int r = 0; r < 3; ++r) covs_out[16 * i + c * 4 + r] = out(r, c);
        }
    }
}

/// one row of 16 floats per interval [i, i + 1] in the layout of sp_imu_deskew_intervals_host, from the per-point functions above;
/// q1_signed_out (4 floats per interval) is the +-q1 the logarithm saw
extern "C" void imu_intervals_restate(const float* traj, uint64_t n_traj, float* rows_out, float* q1_signed_out) {
    for (uint64_t i = 0; i + 1 < n_traj; ++i) {
        const float *e0 = traj + 8 * i, *e1 = e0 + 8;
        Vec4 q0, q1, q1s;
        Vec3 omega;
        for (int k = 0; k < 4; ++k) { q0[k] = e0[k]; q1[k] = e1[k]; }
        slerp_parts(q0, q1, q1s, omega);
        float* row = rows_out + 16 * i;
        row[0] = e0[7];
        row[1] = e1[7];
        for (int k = 0; k < 4; ++k) { row[2 + k] = q0[k]; q1_signed_out[4 * i + k] = q1s[k]; }
        for (int k = 0; k < 3; ++k) {
            row[6 + k] = omega[k];
            row[9 + k] = e0[4 + k];
            row[12 + k] = e1[4 + k] - e0[4 + k];
        }
        row[15] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------ float64, same formula
namespace {
void quat_mult64(const double a[4], const double b[4], double r[4]) {
    r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    r[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
void so3_log64(const double q_in[4], double w[3]) {
    double q[4];
    const double n = std::sqrt(q_in[0] * q_in[0] + q_in[1] * q_in[1] + q_in[2] * q_in[2] + q_in[3] * q_in[3]);
    for (int k = 0; k < 4; ++k) q[k] = n < 1e-6 ? 0.0 : q_in[k] / n;
    if (q[3] < 0.0)
        for (int k = 0; k < 4; ++k) q[k] = -q[k];
    const double vn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    double sc;
    if (vn < 1e-6) sc = 2.0 / q[3] * (1.0 + vn * vn / (6.0 * q[3] * q[3]));
    else if (std::fabs(q[3]) < 1e-6) sc = M_PI / vn;
    else sc = 2.0 * std::atan2(vn, std::fabs(q[3])) / vn;
    for (int k = 0; k < 3; ++k) w[k] = sc * q[k];
}
void so3_exp64(const double w[3], double q[4]) {
    const double theta_sq = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double imag, real;
    if (theta_sq < 1e-6) {
        const double t4 = theta_sq * theta_sq;
        imag = 0.5 - 1.0 / 48.0 * theta_sq + 1.0 / 3840.0 * t4;
        real = 1.0 - 1.0 / 8.0 * theta_sq + 1.0 / 384.0 * t4;
    } else {
        const double theta = std::sqrt(theta_sq);
        imag = std::sin(0.5 * theta) / theta;
        real = std::cos(0.5 * theta);
    }
    q[0] = imag * w[0]; q[1] = imag * w[1]; q[2] = imag * w[2]; q[3] = real;
}
}  // namespace

/// outputs in float64; rows with a non-finite time stamp are copied. The interval is the float32 bisection's (the same decisions
/// as the restatement, so both interpolate the same pair of poses); everything after it is float64.
extern "C" void imu_deskew_f64(const float* points, const float* covs, const float* normals, const float* t_ms, uint64_t n,
                               const float* traj, uint64_t n_traj, double* points_out, double* covs_out, double* normals_out) {
    for (uint64_t i = 0; i < n; ++i) {
        const float* p = points + 4 * i;
        const float t_f = t_ms[i] * 1e-3f;
        if (!std::isfinite(t_f)) {
            for (int k = 0; k < 4; ++k) points_out[4 * i + k] = p[k];
            if (normals) for (int k = 0; k < 4; ++k) normals_out[4 * i + k] = normals[4 * i + k];
            if (covs) for (int k = 0; k < 16; ++k) covs_out[16 * i + k] = covs[16 * i + k];
            continue;
        }
        uint64_t lo, hi;
        bisect(traj, n_traj, t_f, lo, hi);
        const float *e0 = traj + 8 * lo, *e1 = traj + 8 * hi;
        const double t = (double)t_ms[i] * (double)1e-3f, t_lo = e0[7], t_hi = e1[7];
        double alpha = 0.0;
        if (t_hi > t_lo) alpha = std::fmin(std::fmax((t - t_lo) / (t_hi - t_lo), 0.0), 1.0);
        double q0[4], q1[4], q0c[4], dq[4], w[3], dqs[4], q[4];
        double d = 0.0;
        for (int k = 0; k < 4; ++k) { q0[k] = e0[k]; q1[k] = e1[k]; d += q0[k] * q1[k]; }
        if (d < 0.0)
            for (int k = 0; k < 4; ++k) q1[k] = -q1[k];
        q0c[0] = -q0[0]; q0c[1] = -q0[1]; q0c[2] = -q0[2]; q0c[3] = q0[3];
        quat_mult64(q0c, q1, dq);
        so3_log64(dq, w);
        for (int k = 0; k < 3; ++k) w[k] *= alpha;
        so3_exp64(w, dqs);
        quat_mult64(q0, dqs, q);
        const double x = q[0], y = q[1], z = q[2], s = q[3];
        const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - s * z), 2.0 * (x * z + s * y)},
                                {2.0 * (x * y + s * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - s * x)},
                                {2.0 * (x * z - s * y), 2.0 * (y * z + s * x), 1.0 - 2.0 * (x * x + y * y)}};
        for (int r = 0; r < 3; ++r) {
            const double tr = ((double)e1[4 + r] - (double)e0[4 + r]) * alpha + (double)e0[4 + r];
            points_out[4 * i + r] = R[r][0] * p[0] + R[r][1] * p[1] + R[r][2] * p[2] + tr;
        }
        points_out[4 * i + 3] = p[3];
        if (normals) {
            const float* nr = normals + 4 * i;
            for (int r = 0; r < 3; ++r) normals_out[4 * i + r] = R[r][0] * nr[0] + R[r][1] * nr[1] + R[r][2] * nr[2];
            normals_out[4 * i + 3] = 0.0;
        }
        if (covs) {
            const float* C = covs + 16 * i;  // column-major: C(r, c) = C[c * 4 + r]
            double Y[3][3];                  // C3 R^T
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) Y[r][c] = C[0 * 4 + r] * R[c][0] + C[1 * 4 + r] * R[c][1] + C[2 * 4 + r] * R[c][2];
            for (int k = 0; k < 16; ++k) covs_out[16 * i + k] = 0.0;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) covs_out[16 * i + c * 4 + r] = R[r][0] * Y[0][c] + R[r][1] * Y[1][c] + R[r][2] * Y[2][c];
        }
    }
}
