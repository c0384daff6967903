// Host numerics of the per-frame odometry loop: plain host code, no kernel in this file.
//   MotionPredictor / AdaptiveMotionPredictor::predict (pipeline/motion_predictor.hpp:60-76, adaptive_motion_predictor.hpp:54-133)
//   the velocity of a pose pair (pipeline/lidar_odometry.hpp:282-286)
//   Submap::is_keyframe (pipeline/submapping.hpp:144-161)
//   imu::estimate_initial_alignment and detail::yaw_from_rotation (algorithms/imu/imu_initial_alignment.hpp:85-218)
// The reference runs all of it on the host with Eigen, once per scan. Eigen's SelfAdjointEigenSolver<Matrix3f>, AngleAxisf,
// Quaternionf and FromTwoVectors are third-party arithmetic the reference does not pin: here they are this
// project's own helpers (eigen_sym3, rot_to_angle_axis, rot_to_quat, quat_mult of sp_pose_math.h; so3_exp, quat_to_rot of
// sp_math.h), matrix products are plain multiply-add sums with k ascending.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sp_common.h"
#include "sp_math.h"
#include "sp_pose_math.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

int odometry_invalid(const char* msg) {
    sp_set_error(msg);
    return SP_ERR_INVALID_ARGUMENT;
}

// adaptive_motion_predictor.hpp:62-74 / :84-94 for the 3x3 block of H_raw at (o, o)
float degeneracy_factor(const sp_motion_axis_params& axis, const float* H, int o, uint32_t inlier) {
    float blk[3][3], lam[3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) blk[i][j] = H[(o + i) * 6 + (o + j)];
    eigen_sym3(blk, lam, V);
    const float min_eig_ratio = lam[0] / (float)inlier;
    const float score =
        std::clamp((min_eig_ratio - axis.min_eigenvalue_low) / std::max(axis.min_eigenvalue_high - axis.min_eigenvalue_low, 1e-6f), 0.0f, 1.0f);
    return axis.factor_max * (1.0f - score) + axis.factor_min * score;
}

void normalize4(float q[4]) {
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (n > 0.0f)
        for (int i = 0; i < 4; ++i) q[i] /= n;
}

// Quaternionf::FromTwoVectors (Eigen/src/Geometry/Quaternion.h) for unit vectors; see sycl_points_amd.h for the opposite case
void quat_from_two_vectors(const float v0[3], const float v1[3], float q[4]) {
    float c = v1[0] * v0[0] + v1[1] * v0[1] + v1[2] * v0[2];
    if (c < -1.0f + 1e-5f) {
        c = std::max(c, -1.0f);
        int least = 0;
        for (int i = 1; i < 3; ++i)
            if (fabsf(v0[i]) < fabsf(v0[least])) least = i;
        float e[3] = {0.0f, 0.0f, 0.0f};
        e[least] = 1.0f;
        float axis[3] = {v0[1] * e[2] - v0[2] * e[1], v0[2] * e[0] - v0[0] * e[2], v0[0] * e[1] - v0[1] * e[0]};
        const float an = sqrtf(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
        const float w2 = (1.0f + c) * 0.5f;
        const float s = sqrtf(1.0f - w2) / an;
        q[0] = axis[0] * s; q[1] = axis[1] * s; q[2] = axis[2] * s; q[3] = sqrtf(w2);
        return;
    }
    const float axis[3] = {v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]};
    const float s = sqrtf((1.0f + c) * 2.0f);
    const float invs = 1.0f / s;
    q[0] = axis[0] * invs; q[1] = axis[1] * invs; q[2] = axis[2] * invs; q[3] = s * 0.5f;
}

}  // namespace
}  // namespace sp

extern "C" int sp_motion_predict_host(const sp_motion_predict_params* params, sp_motion_predict_state* state,
                                      const float* linear_velocity3, const float* angular_velocity_rotvec3, const float* odom16,
                                      float dt, const float* H_raw36_rowmajor, uint32_t inlier, int registrated,
                                      const float* gyro_delta_rotation9, const float* imu_se3_pose16, float* T_pred16_out,
                                      float* factors2_out) {
    if (!params || !state || !linear_velocity3 || !angular_velocity_rotvec3 || !odom16 || !T_pred16_out)
        return sp::odometry_invalid("[sp_motion_predict_host] null argument");
    if (registrated && inlier > 0 && !H_raw36_rowmajor) return sp::odometry_invalid("[sp_motion_predict_host] H_raw is null");
    if (params->mode == SP_MOTION_IMU_SE3 && imu_se3_pose16) {  // motion_predictor.hpp:64-66
        std::memcpy(T_pred16_out, imu_se3_pose16, 16 * sizeof(float));
        if (factors2_out) { factors2_out[0] = params->rotation.factor_max; factors2_out[1] = params->translation.factor_max; }
        return SP_OK;
    }
    float rot_factor = params->rotation.factor_max, trans_factor = params->translation.factor_max;
    if (registrated && inlier > 0) {
        rot_factor = sp::degeneracy_factor(params->rotation, H_raw36_rowmajor, 0, inlier);
        trans_factor = sp::degeneracy_factor(params->translation, H_raw36_rowmajor, 3, inlier);
    }
    if (factors2_out) { factors2_out[0] = rot_factor; factors2_out[1] = trans_factor; }
    // :103-113 the moving averages, component by component
    const float alpha = params->velocity_ema_alpha;
    for (int i = 0; i < 3; ++i) {
        state->linear[i] = state->has_linear ? alpha * linear_velocity3[i] + (1.0f - alpha) * state->linear[i] : linear_velocity3[i];
        state->angular[i] =
            state->has_angular ? alpha * angular_velocity_rotvec3[i] + (1.0f - alpha) * state->angular[i] : angular_velocity_rotvec3[i];
    }
    state->has_linear = state->has_angular = 1;
    // :115-127
    const float* w = state->angular;
    const float ang_norm = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    float rotvec[3] = {0.0f, 0.0f, 0.0f};
    if (ang_norm > 1e-6f) {
        const float angle = ang_norm * dt * rot_factor;
        for (int i = 0; i < 3; ++i) rotvec[i] = (w[i] / ang_norm) * angle;
    }
    const sp::Rigid odom = sp::load_rigid_colmajor(odom16);
    sp::Rigid pred;
    for (int i = 0; i < 3; ++i) {
        float s = 0.0f;
        for (int k = 0; k < 3; ++k) s += odom.R[i][k] * (state->linear[k] * dt * trans_factor);
        pred.t[i] = odom.t[i] + s;
    }
    float q_odom[4], q_delta[4], q[4];
    sp::rot_to_quat(odom.R, q_odom);
    sp::so3_exp(rotvec, q_delta);
    sp::quat_mult(q_odom, q_delta, q);
    sp::normalize4(q);
    sp::quat_to_rot(q, pred.R);
    if (params->mode == SP_MOTION_GYRO_LIDAR_CV && gyro_delta_rotation9) {  // motion_predictor.hpp:70-74
        sp::Rigid rel = sp::rigid_mul(sp::rigid_inverse(odom), pred);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) rel.R[i][j] = gyro_delta_rotation9[j * 3 + i];
        pred = sp::rigid_mul(odom, rel);
    }
    sp::store_rigid_colmajor(pred, T_pred16_out);
    return SP_OK;
}

extern "C" int sp_velocity_from_poses_host(const float* T_prev16, const float* T_cur16, float dt, float* linear3_out,
                                           float* angle_axis4_out) {
    if (!T_prev16 || !T_cur16 || !linear3_out || !angle_axis4_out) return sp::odometry_invalid("[sp_velocity_from_poses_host] null argument");
    const sp::Rigid delta = sp::rigid_mul(sp::rigid_inverse(sp::load_rigid_colmajor(T_prev16)), sp::load_rigid_colmajor(T_cur16));
    float angle;
    sp::rot_to_angle_axis(delta.R, &angle, angle_axis4_out + 1);
    angle_axis4_out[0] = angle / dt;
    for (int i = 0; i < 3; ++i) linear3_out[i] = delta.t[i] / dt;
    return SP_OK;
}

extern "C" int sp_keyframe_decision_host(const float* T_last_keyframe16, const float* T_current16, double last_keyframe_time,
                                         double timestamp, float distance_threshold, float angle_threshold_degrees,
                                         float time_threshold_seconds, int* is_keyframe_out, double* metrics3_out) {
    if (!T_last_keyframe16 || !T_current16 || !is_keyframe_out) return sp::odometry_invalid("[sp_keyframe_decision_host] null argument");
    const sp::Rigid delta =
        sp::rigid_mul(sp::rigid_inverse(sp::load_rigid_colmajor(T_last_keyframe16)), sp::load_rigid_colmajor(T_current16));
    const float distance = sqrtf(delta.t[0] * delta.t[0] + delta.t[1] * delta.t[1] + delta.t[2] * delta.t[2]);
    float angle_rad, axis[3];
    sp::rot_to_angle_axis(delta.R, &angle_rad, axis);
    const float angle = fabsf(angle_rad) * (180.0f / sp::kPi);
    const double delta_time = last_keyframe_time > 0.0 ? timestamp - last_keyframe_time : DBL_MAX;
    *is_keyframe_out = (distance >= distance_threshold || angle >= angle_threshold_degrees ||
                        delta_time >= (double)time_threshold_seconds)
                           ? 1
                           : 0;
    if (metrics3_out) { metrics3_out[0] = distance; metrics3_out[1] = angle; metrics3_out[2] = delta_time; }
    return SP_OK;
}

extern "C" float sp_yaw_from_rotation_host(const float* R9_colmajor) {
    if (!R9_colmajor) return 0.0f;
    const float cy = R9_colmajor[0], sy = R9_colmajor[1];
    if ((cy * cy + sy * sy) < 1e-12f) return 0.0f;
    return atan2f(sy, cy);
}

extern "C" int sp_initial_alignment_host(const double* stamps_host, const float* gyro_accel_host, size_t n, const float* gravity3,
                                         const sp_initial_alignment_params* params, const float* bias6, int bypass_stationarity,
                                         sp_initial_alignment_result* result_out) {
    if (!gravity3 || !params || !bias6 || !result_out || (n > 0 && (!stamps_host || !gyro_accel_host)))
        return sp::odometry_invalid("[sp_initial_alignment_host] null argument");
    sp_initial_alignment_result& res = *result_out;
    std::memset(&res, 0, sizeof res);
    res.R_world_imu[0] = res.R_world_imu[4] = res.R_world_imu[8] = 1.0f;
    auto fail = [&](const char* msg) {
        std::snprintf(res.error_message, sizeof res.error_message, "%s", msg);
        return SP_OK;
    };
    const float gravity_norm = sqrtf(gravity3[0] * gravity3[0] + gravity3[1] * gravity3[1] + gravity3[2] * gravity3[2]);
    if (gravity_norm < 1e-3f) return fail("gravity vector is (near) zero");
    if (n < 2) return fail("IMU buffer has fewer than 2 samples");
    const double t_end = stamps_host[n - 1];
    const double buffer_span = t_end - stamps_host[0];
    if (buffer_span + 1e-6 < (double)params->required_duration_sec) return fail("IMU buffer spans less than required_duration_sec");
    // :113-132 the window, with the one earlier sample that makes its span reach `required`
    const double t_required_start = t_end - (double)params->required_duration_sec;
    std::vector<size_t> window;
    window.reserve(n);
    bool has_pre = false;
    size_t pre_sample = 0;
    for (size_t i = 0; i < n; ++i) {
        if (stamps_host[i] >= t_required_start) window.push_back(i);
        else { pre_sample = i; has_pre = true; }
    }
    if (window.empty()) return fail("no IMU samples in required window");
    if (has_pre && stamps_host[window.front()] > t_required_start + 1e-6) window.insert(window.begin(), pre_sample);
    res.window_size = (int)window.size();
    // :134-162 means and variances in double
    double gyro_mean[3] = {0, 0, 0}, accel_mean[3] = {0, 0, 0}, gyro_var[3] = {0, 0, 0}, accel_var[3] = {0, 0, 0};
    for (size_t i : window)
        for (int k = 0; k < 3; ++k) {
            gyro_mean[k] += (double)gyro_accel_host[i * 6 + k];
            accel_mean[k] += (double)gyro_accel_host[i * 6 + 3 + k];
        }
    const double cnt = (double)window.size();
    for (int k = 0; k < 3; ++k) { gyro_mean[k] /= cnt; accel_mean[k] /= cnt; }
    for (size_t i : window)
        for (int k = 0; k < 3; ++k) {
            const double dg = (double)gyro_accel_host[i * 6 + k] - gyro_mean[k], da = (double)gyro_accel_host[i * 6 + 3 + k] - accel_mean[k];
            gyro_var[k] += dg * dg;
            accel_var[k] += da * da;
        }
    for (int k = 0; k < 3; ++k) {
        res.gyro_std[k] = (float)std::sqrt(gyro_var[k] / cnt);
        res.accel_std[k] = (float)std::sqrt(accel_var[k] / cnt);
        res.accel_mean[k] = (float)accel_mean[k];
    }
    res.accel_norm = (float)std::sqrt(accel_mean[0] * accel_mean[0] + accel_mean[1] * accel_mean[1] + accel_mean[2] * accel_mean[2]);
    if (!bypass_stationarity) {  // :165-179
        for (int k = 0; k < 3; ++k)
            if (res.gyro_std[k] > params->max_gyro_std) return fail("gyro_std exceeds threshold (robot not stationary?)");
        for (int k = 0; k < 3; ++k)
            if (res.accel_std[k] > params->max_accel_std) return fail("accel_std exceeds threshold (robot not stationary?)");
        if (fabsf(res.accel_norm - gravity_norm) > params->max_accel_norm_error)
            return fail("|a_mean| - |gravity| exceeds threshold (unmodelled accel bias?)");
    }
    // :181-195
    float a[3];
    for (int k = 0; k < 3; ++k) a[k] = res.accel_mean[k] - bias6[3 + k];
    const float a_norm = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (a_norm < 1e-3f) return fail("bias-corrected accel magnitude is (near) zero");
    float body_up[3], world_up[3], q[4], R[3][3];
    for (int k = 0; k < 3; ++k) { body_up[k] = a[k] / a_norm; world_up[k] = -gravity3[k] / gravity_norm; }
    sp::quat_from_two_vectors(body_up, world_up, q);
    sp::normalize4(q);
    sp::quat_to_rot(q, R);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) res.R_world_imu[j * 3 + i] = R[i][j];
    res.roll_rad = atan2f(R[2][1], R[2][2]);  // :198-199
    res.pitch_rad = asinf(-std::clamp(R[2][0], -1.0f, 1.0f));
    for (int k = 0; k < 3; ++k) res.gyro_bias[k] = params->estimate_gyro_bias ? (float)gyro_mean[k] : bias6[k];
    res.success = 1;
    return SP_OK;
}
