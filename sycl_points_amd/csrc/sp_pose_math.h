// Host-side pose algebra shared by the pose-space terms of Registration::align (pose_terms.hip) and the relative twist of
// the constant-velocity deskew (deskew.hip): quaternion of a rotation, so3_log, se3_log, the inverse of an isometry; the
// quaternion product of the IMU code, the angle-axis of a rotation and the symmetric 3x3 eigen-solver of the degenerate
// regularisation, which the odometry's host numerics (odometry_host.hip) share.
// Plain host arithmetic in the reference's order (the reference runs these on the host with Eigen).
#pragma once
#include <cmath>
#include <cstring>

#include "sp_math.h"

namespace sp {

// rotation_matrix_to_quaternion (eigen_utils.hpp:774-806), quaternion as x,y,z,w
inline void rot_to_quat(const float R[3][3], float q[4]) {
    const float tr = R[0][0] + R[1][1] + R[2][2];
    if (tr > 0.0f) {
        const float S = sqrtf(tr + 1.0f) * 2.0f;
        q[0] = (R[2][1] - R[1][2]) / S; q[1] = (R[0][2] - R[2][0]) / S; q[2] = (R[1][0] - R[0][1]) / S; q[3] = 0.25f * S;
    } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
        const float S = sqrtf(1.0f + R[0][0] - R[1][1] - R[2][2]) * 2.0f;
        q[0] = 0.25f * S; q[1] = (R[0][1] + R[1][0]) / S; q[2] = (R[0][2] + R[2][0]) / S; q[3] = (R[2][1] - R[1][2]) / S;
    } else if (R[1][1] > R[2][2]) {
        const float S = sqrtf(1.0f + R[1][1] - R[0][0] - R[2][2]) * 2.0f;
        q[0] = (R[0][1] + R[1][0]) / S; q[1] = 0.25f * S; q[2] = (R[1][2] + R[2][1]) / S; q[3] = (R[0][2] - R[2][0]) / S;
    } else {
        const float S = sqrtf(1.0f + R[2][2] - R[0][0] - R[1][1]) * 2.0f;
        q[0] = (R[0][2] + R[2][0]) / S; q[1] = (R[1][2] + R[2][1]) / S; q[2] = 0.25f * S; q[3] = (R[1][0] - R[0][1]) / S;
    }
}

// so3_log (eigen_utils.hpp:948-986)
inline void so3_log(const float q_in[4], float w_out[3]) {
    float q[4];
    const float n = sqrtf(fmaf(q_in[3], q_in[3], fmaf(q_in[2], q_in[2], fmaf(q_in[1], q_in[1], q_in[0] * q_in[0]))));
    for (int i = 0; i < 4; ++i) q[i] = (n < 1e-6f) ? 0.0f : q_in[i] * (1.0f / n);
    if (q[3] < 0.0f)
        for (int i = 0; i < 4; ++i) q[i] = -q[i];
    const float w = q[3];
    const float vn = sqrtf(chain3(q[0], q[0], q[1], q[1], q[2], q[2]));
    float scale;
    if (vn < 1e-6f) scale = 2.0f / w * (1.0f + vn * vn / (6.0f * w * w));
    else if (fabsf(w) < 1e-6f) scale = kPi / vn;
    else scale = 2.0f * atan2f(vn, fabsf(w)) / vn;
    for (int i = 0; i < 3; ++i) w_out[i] = scale * q[i];
}

// se3_log (eigen_utils.hpp:991-1034), rotation-first twist
inline void se3_log(const Rigid& T, float a[6]) {
    float q[4], w[3];
    rot_to_quat(T.R, q);
    so3_log(q, w);
    const float theta = sqrtf(chain3(w[0], w[0], w[1], w[1], w[2], w[2]));
    const float O[3][3] = {{0.0f, -w[2], w[1]}, {w[2], 0.0f, -w[0]}, {-w[1], w[0], 0.0f}};
    float Vi[3][3];
    float coeff = 0.0f;
    if (!(theta < 1e-6f)) {
        const float half = 0.5f * theta;
        coeff = (1.0f - theta * cosf(half) / (2.0f * sinf(half))) / (theta * theta);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float o2 = 0.0f;
            for (int k = 0; k < 3; ++k) o2 += O[i][k] * O[k][j];
            Vi[i][j] = ((i == j) ? 1.0f : 0.0f) - 0.5f * O[i][j];
            if (!(theta < 1e-6f)) Vi[i][j] += coeff * o2;
        }
    for (int i = 0; i < 3; ++i) {
        a[i] = w[i];
        float s = 0.0f;
        for (int k = 0; k < 3; ++k) s += Vi[i][k] * T.t[k];
        a[3 + i] = s;
    }
}

inline Rigid rigid_inverse(const Rigid& T) {  // Isometry3f::inverse(): R^T, -R^T t
    Rigid o;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o.R[i][j] = T.R[j][i];
    }
    for (int i = 0; i < 3; ++i) {
        float s = 0.0f;
        for (int k = 0; k < 3; ++k) s += o.R[i][k] * T.t[k];
        o.t[i] = -s;
    }
    return o;
}


// quat_mult (imu_deskew.hpp:43-50)
inline void quat_mult(const float a[4], const float b[4], float r[4]) {
    r[0] = fmaf(a[3], b[0], fmaf(+a[0], b[3], fmaf(+a[1], b[2], -a[2] * b[1])));
    r[1] = fmaf(a[3], b[1], fmaf(-a[0], b[2], fmaf(+a[1], b[3], +a[2] * b[0])));
    r[2] = fmaf(a[3], b[2], fmaf(+a[0], b[1], fmaf(-a[1], b[0], +a[2] * b[3])));
    r[3] = fmaf(a[3], b[3], fmaf(-a[0], b[0], fmaf(-a[1], b[1], -a[2] * b[2])));
}

// Eigen::AngleAxisf(Matrix3f) (Eigen/src/Geometry/AngleAxis.h, through the quaternion): angle = 2 atan2(|v|, |w|) >= 0, the
// axis v / |v| turned round when w < 0; angle 0 about the x axis for the identity.
inline void rot_to_angle_axis(const float R[3][3], float* angle, float axis[3]) {
    float q[4];
    rot_to_quat(R, q);
    float vn = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    *angle = 0.0f;
    axis[0] = 1.0f; axis[1] = 0.0f; axis[2] = 0.0f;
    if (vn != 0.0f) {
        *angle = 2.0f * atan2f(vn, fabsf(q[3]));
        if (q[3] < 0.0f) vn = -vn;
        for (int i = 0; i < 3; ++i) axis[i] = q[i] / vn;
    }
}

// Symmetric 3x3 eigen-pairs by cyclic Jacobi rotations (stands in for Eigen::SelfAdjointEigenSolver<Matrix3f>,
// degenerate_regularization.hpp:71-78): ascending eigenvalues, unit eigenvectors in the columns of V.
inline void eigen_sym3(const float A_in[3][3], float lam[3], float V[3][3]) {
    float A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            A[i][j] = 0.5f * (A_in[i][j] + A_in[j][i]);
            V[i][j] = (i == j) ? 1.0f : 0.0f;
        }
    for (int sweep = 0; sweep < 32; ++sweep) {
        const float off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const float dg = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (!(off > 1e-18f * dg)) break;
        static const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
        for (int e = 0; e < 3; ++e) {
            const int p = P[e], q = Q[e];
            if (A[p][q] == 0.0f) continue;
            const float tau = (A[q][q] - A[p][p]) / (2.0f * A[p][q]);
            const float t = copysignf(1.0f, tau) / (fabsf(tau) + sqrtf(fmaf(tau, tau, 1.0f)));
            const float c = 1.0f / sqrtf(fmaf(t, t, 1.0f)), s = t * c;
            for (int k = 0; k < 3; ++k) {
                const float x = A[k][p], y = A[k][q];
                A[k][p] = c * x - s * y;
                A[k][q] = s * x + c * y;
            }
            for (int k = 0; k < 3; ++k) {
                const float x = A[p][k], y = A[q][k];
                A[p][k] = c * x - s * y;
                A[q][k] = s * x + c * y;
            }
            for (int k = 0; k < 3; ++k) {
                const float x = V[k][p], y = V[k][q];
                V[k][p] = c * x - s * y;
                V[k][q] = s * x + c * y;
            }
        }
    }
    int idx[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (A[idx[j]][idx[j]] < A[idx[i]][idx[i]]) { const int t = idx[i]; idx[i] = idx[j]; idx[j] = t; }
    float Vs[3][3];
    for (int c = 0; c < 3; ++c) {
        lam[c] = A[idx[c]][idx[c]];
        for (int r = 0; r < 3; ++r) Vs[r][c] = V[r][idx[c]];
    }
    std::memcpy(V, Vs, sizeof(Vs));
}

}  // namespace sp
