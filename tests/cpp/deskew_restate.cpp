// CPU restatement of the constant-velocity deskew (deskew/relative_pose_deskew.hpp:120-172), float32 with the explicit fmaf
// chains of eigen_utils.hpp (oracle/oracle_math.hpp, pinned by tests/test_oracle_pins.py), and a float64 evaluation of the
// same formula as the yardstick of both. Built by the tests with g++ -O2 -ffp-contract=off as a shared library.
//
// Unlike the reference, both read a row completely before they write it, so the outputs may be the inputs (the library's
// documented deviation: the reference zeroes normals_out / covs_out first and returns zeros in place).
#include <cmath>
#include <cstdint>

#include "../../oracle/oracle_math.hpp"

using namespace oracle;

extern "C" void deskew_restate(const float* points, const float* covs, const float* normals, const float* t_ms, uint64_t n,
                               const float* twist6, float duration, float* points_out, float* covs_out, float* normals_out) {
    for (uint64_t i = 0; i < n; ++i) {
        Vec4 p, nr;
        Mat4 C;
        for (int k = 0; k < 4; ++k) p[k] = points[4 * i + k];
        if (normals) for (int k = 0; k < 4; ++k) nr[k] = normals[4 * i + k];
        if (covs) for (int k = 0; k < 16; ++k) C[k] = covs[16 * i + k];
        const float ts = t_ms[i] * 1e-3f;
        if (!std::isfinite(ts)) {
            for (int k = 0; k < 4; ++k) points_out[4 * i + k] = p[k];
            if (normals) for (int k = 0; k < 4; ++k) normals_out[4 * i + k] = nr[k];
            if (covs) for (int k = 0; k < 16; ++k) covs_out[16 * i + k] = C[k];
            continue;
        }
        const float tau = std::fmin(std::fmax(ts / duration, 0.0f), 1.0f);  // sycl::clamp
        Vec6 a;
        for (int k = 0; k < 6; ++k) a[k] = twist6[k] * tau;
        const Mat4 M = se3_exp(a);
        const Vec4 q = matvec<4, 4>(M, p);
        for (int k = 0; k < 4; ++k) points_out[4 * i + k] = q[k];
        Vec3 w;
        for (int k = 0; k < 3; ++k) w[k] = a[k];
        const Mat3 R = quaternion_to_rotation_matrix(so3_exp(w));
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

// ------------------------------------------------------------------------------------------------ float64, same formula
namespace {
struct Rot64 {
    double R[3][3];
};
Rot64 rotation64(const double w[3]) {  // quaternion_to_rotation_matrix(so3_exp(w))
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
    const double x = imag * w[0], y = imag * w[1], z = imag * w[2], s = real;
    Rot64 o;
    o.R[0][0] = 1.0 - 2.0 * (y * y + z * z); o.R[0][1] = 2.0 * (x * y - s * z);       o.R[0][2] = 2.0 * (x * z + s * y);
    o.R[1][0] = 2.0 * (x * y + s * z);       o.R[1][1] = 1.0 - 2.0 * (x * x + z * z); o.R[1][2] = 2.0 * (y * z - s * x);
    o.R[2][0] = 2.0 * (x * z - s * y);       o.R[2][1] = 2.0 * (y * z + s * x);       o.R[2][2] = 1.0 - 2.0 * (x * x + y * y);
    return o;
}
}  // namespace

/// outputs in float64; rows with a non-finite time stamp are copied
extern "C" void deskew_f64(const float* points, const float* covs, const float* normals, const float* t_ms, uint64_t n,
                           const float* twist6, float duration, double* points_out, double* covs_out, double* normals_out) {
    for (uint64_t i = 0; i < n; ++i) {
        const float* p = points + 4 * i;
        const double ts = (double)t_ms[i] * (double)1e-3f;
        if (!std::isfinite(ts)) {
            for (int k = 0; k < 4; ++k) points_out[4 * i + k] = p[k];
            if (normals) for (int k = 0; k < 4; ++k) normals_out[4 * i + k] = normals[4 * i + k];
            if (covs) for (int k = 0; k < 16; ++k) covs_out[16 * i + k] = covs[16 * i + k];
            continue;
        }
        const double tau = std::fmin(std::fmax(ts / (double)duration, 0.0), 1.0);
        double a[6];
        for (int k = 0; k < 6; ++k) a[k] = (double)twist6[k] * tau;
        const Rot64 Rm = rotation64(a);
        const double theta_sq = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], theta = std::sqrt(theta_sq);
        double V[3][3];
        if (theta < 1e-6) {
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) V[r][c] = Rm.R[r][c];
        } else {
            const double O[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
            const double A = (1.0 - std::cos(theta)) / theta_sq, B = (theta - std::sin(theta)) / (theta_sq * theta);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    double o2 = 0.0;
                    for (int k = 0; k < 3; ++k) o2 += O[r][k] * O[k][c];
                    V[r][c] = (r == c ? 1.0 : 0.0) + O[r][c] * A + o2 * B;
                }
        }
        for (int r = 0; r < 3; ++r) {
            const double t = V[r][0] * a[3] + V[r][1] * a[4] + V[r][2] * a[5];
            points_out[4 * i + r] = Rm.R[r][0] * p[0] + Rm.R[r][1] * p[1] + Rm.R[r][2] * p[2] + t * p[3];
        }
        points_out[4 * i + 3] = p[3];
        if (normals) {
            const float* nr = normals + 4 * i;
            for (int r = 0; r < 3; ++r) normals_out[4 * i + r] = Rm.R[r][0] * nr[0] + Rm.R[r][1] * nr[1] + Rm.R[r][2] * nr[2];
            normals_out[4 * i + 3] = 0.0;
        }
        if (covs) {
            const float* C = covs + 16 * i;  // column-major: C(r, c) = C[c * 4 + r]
            double Y[3][3];                  // C3 R^T
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) Y[r][c] = C[0 * 4 + r] * Rm.R[c][0] + C[1 * 4 + r] * Rm.R[c][1] + C[2 * 4 + r] * Rm.R[c][2];
            for (int k = 0; k < 16; ++k) covs_out[16 * i + k] = 0.0;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c)
                    covs_out[16 * i + c * 4 + r] = Rm.R[r][0] * Y[0][c] + Rm.R[r][1] * Y[1][c] + Rm.R[r][2] * Y[2][c];
        }
    }
}

/// se3_log(prev^-1 * cur) in float32 as the reference's host code forms it (oracle_math.hpp), for the known answer
extern "C" void relative_twist_restate(const float* prev16, const float* cur16, float* twist6) {
    Mat4 P, Cm, Pinv = Mat4::Identity();
    for (int k = 0; k < 16; ++k) { P[k] = prev16[k]; Cm[k] = cur16[k]; }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Pinv(i, j) = P(j, i);
    for (int i = 0; i < 3; ++i) Pinv(i, 3) = -(Pinv(i, 0) * P(0, 3) + Pinv(i, 1) * P(1, 3) + Pinv(i, 2) * P(2, 3));
    const Vec6 t = se3_log(isometry_mul(Pinv, Cm));
    for (int k = 0; k < 6; ++k) twist6[k] = t[k];
}
