// Host-side pose algebra shared by the pose-space terms of Registration::align (pose_terms.hip) and the relative twist of
// the constant-velocity deskew (deskew.hip): quaternion of a rotation, so3_log, se3_log, the inverse of an isometry.
// Plain host arithmetic in the reference's order (the reference runs these on the host with Eigen).
#pragma once
#include <cmath>

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

}  // namespace sp
