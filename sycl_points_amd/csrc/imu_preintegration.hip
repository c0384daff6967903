// IMU preintegration and the host half of the IMU deskew: plain host code, no kernel in this file.
//   imu::IMUPreintegration (algorithms/imu/imu_preintegration.hpp:180-529) as the opaque handle sp_imu_preint_*;
//   steps 1-3 of deskew::deskew_point_cloud_imu (algorithms/deskew/imu_deskew.hpp:158-285) as sp_imu_deskew_trajectory_host;
//   the per-interval constants of the kernel (imu_deskew.hpp:54-89, 376-386) as sp_imu_deskew_intervals_host.
// The reference runs all of it on the host too (tens of samples per scan).
//
// Eigen: the reference writes these recurrences as Eigen expressions, whose evaluation order (and whose matrix ->
// quaternion conversion) is third-party arithmetic the reference does not pin. Here every matrix product
// is a plain multiply-add sum with k ascending, every chain of factors is evaluated left to right as written, and every
// conversion between rotations and quaternions goes through this project's own helpers (so3_exp / quat_to_rot of
// sp_math.h, rot_to_quat / so3_log of sp_pose_math.h) - also where the reference calls Eigen::Quaternionf(Matrix3f)
// (imu_deskew.hpp:265).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "sp_common.h"
#include "sp_math.h"
#include "sp_pose_math.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

struct M3 {
    float m[3][3];
};
inline M3 identity3() { return M3{{{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}}}; }
inline M3 zero3() { return M3{{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}}}; }
inline M3 mul(const M3& A, const M3& B) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 3; ++k) s += A.m[i][k] * B.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}
inline M3 transposed(const M3& A) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = A.m[j][i];
    return r;
}
inline M3 scaled(const M3& A, float s) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = A.m[i][j] * s;
    return r;
}
inline M3 add(const M3& A, const M3& B) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = A.m[i][j] + B.m[i][j];
    return r;
}
inline M3 sub(const M3& A, const M3& B) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = A.m[i][j] - B.m[i][j];
    return r;
}
inline void mulv(const M3& A, const float v[3], float out[3]) {
    for (int i = 0; i < 3; ++i) {
        float s = 0.0f;
        for (int k = 0; k < 3; ++k) s += A.m[i][k] * v[k];
        out[i] = s;
    }
}
inline M3 skew(const float x[3]) {  // eigen_utils::lie::skew
    return M3{{{0.0f, -x[2], x[1]}, {x[2], 0.0f, -x[0]}, {-x[1], x[0], 0.0f}}};
}
inline M3 rotation_of(const float phi[3]) {  // quaternion_to_rotation_matrix(so3_exp(phi))
    float q[4];
    M3 R;
    so3_exp(phi, q);
    quat_to_rot(q, R.m);
    return R;
}
inline M3 load_colmajor3(const float* a) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[i][j] = a[j * 3 + i];
    return r;
}
inline void store_colmajor3(const M3& A, float* a) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[j * 3 + i] = A.m[i][j];
}

// right_jacobian_so3 (imu_preintegration.hpp:340-353)
inline M3 right_jacobian_so3(const float phi[3]) {
    const float theta = sqrtf(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    const M3 S = skew(phi);
    const M3 S2 = mul(S, S);
    if (theta < 1e-4f) return add(sub(identity3(), scaled(S, 0.5f)), scaled(S2, 1.0f / 6.0f));
    return add(sub(identity3(), scaled(S, (1.0f - cosf(theta)) / (theta * theta))),
               scaled(S2, (theta - sinf(theta)) / (theta * theta * theta)));
}

struct Sample {
    double timestamp = 0.0;
    float gyro[3] = {0.0f, 0.0f, 0.0f};
    float accel[3] = {0.0f, 0.0f, 0.0f};
};

struct State {  // PreintegrationResult (:109-135); matrices row-major here, column-major at the C ABI
    M3 Delta_R = identity3();
    float Delta_v[3] = {0.0f, 0.0f, 0.0f};
    float Delta_p[3] = {0.0f, 0.0f, 0.0f};
    double dt_total = 0.0;
    M3 J_R_bg = zero3(), J_v_bg = zero3(), J_v_ba = zero3(), J_p_bg = zero3(), J_p_ba = zero3();
    float cov[15][15] = {};
};

inline void set_block(float M[15][15], int r0, int c0, const M3& B) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[r0 + i][c0 + j] = B.m[i][j];
}

struct Preint {
    sp_imu_params params;
    float bias_gyro[3] = {0.0f, 0.0f, 0.0f}, bias_accel[3] = {0.0f, 0.0f, 0.0f};  // the linearisation point
    State result;
    M3 R_world_body_at_reset = identity3();
    Sample prev;
    bool has_prev = false;
    int num_measurements = 0;
    int step_count = 0;

    void reset(const float* bias6, const float* cov225, const float* R9) {  // :202-212
        for (int k = 0; k < 3; ++k) {
            bias_gyro[k] = bias6 ? bias6[k] : 0.0f;
            bias_accel[k] = bias6 ? bias6[3 + k] : 0.0f;
        }
        result = State{};
        if (cov225)
            for (int i = 0; i < 15; ++i)
                for (int j = 0; j < 15; ++j) result.cov[i][j] = cov225[j * 15 + i];
        R_world_body_at_reset = R9 ? load_colmajor3(R9) : identity3();
        has_prev = false;
        num_measurements = 0;
        step_count = 0;
    }

    void integrate(const Sample& meas) {  // :217-230
        if (!has_prev) {  // the first sample only primes the integrator
            prev = meas;
            has_prev = true;
            ++num_measurements;
            return;
        }
        if (meas.timestamp <= prev.timestamp) return;  // dropped, prev stays
        integrate_step(prev, meas);
        prev = meas;
        ++num_measurements;
    }

    void integrate_step(const Sample& m0, const Sample& m1) {  // :356-519
        const double dt = m1.timestamp - m0.timestamp;
        if (dt < 1e-9) return;
        const float dt_f = static_cast<float>(dt);
        float omega_mid[3], a_mid[3], phi_mid[3], phi_half[3];
        for (int k = 0; k < 3; ++k) {
            const float omega_0 = m0.gyro[k] - bias_gyro[k], omega_1 = m1.gyro[k] - bias_gyro[k];
            const float a_0 = m0.accel[k] * params.accel_scale - bias_accel[k];
            const float a_1 = m1.accel[k] * params.accel_scale - bias_accel[k];
            omega_mid[k] = 0.5f * (omega_0 + omega_1);
            a_mid[k] = 0.5f * (a_0 + a_1);
            phi_mid[k] = omega_mid[k] * dt_f;
            phi_half[k] = omega_mid[k] * (0.5f * dt_f);
        }
        const M3 R_step = rotation_of(phi_mid);
        const M3 R_half = rotation_of(phi_half);
        const M3 Delta_R_mid = mul(result.Delta_R, R_half);

        const M3 J_R_bg_old = result.J_R_bg, J_v_bg_old = result.J_v_bg, J_v_ba_old = result.J_v_ba;
        float a_nav[3];
        mulv(Delta_R_mid, a_mid, a_nav);

        // --- state (Delta_p reads the velocity of before the step)
        result.Delta_R = mul(result.Delta_R, R_step);
        for (int k = 0; k < 3; ++k) {
            const float v_old = result.Delta_v[k];
            result.Delta_p[k] += v_old * dt_f + 0.5f * a_nav[k] * dt_f * dt_f;
            result.Delta_v[k] = v_old + a_nav[k] * dt_f;
        }
        result.dt_total += dt;

        // --- bias Jacobians
        const M3 Jr = right_jacobian_so3(phi_mid);
        const M3 Jr_half = right_jacobian_so3(phi_half);
        const M3 skew_a = skew(a_mid);
        const M3 R_half_t = transposed(R_half);
        const M3 J_R_mid_bg = sub(mul(R_half_t, J_R_bg_old), scaled(Jr_half, 0.5f * dt_f));
        result.J_R_bg = sub(mul(transposed(R_step), J_R_bg_old), scaled(Jr, dt_f));
        const M3 RSJ = mul(mul(Delta_R_mid, skew_a), J_R_mid_bg);  // Delta_R_mid * skew_a * J_R_mid_bg, left to right
        result.J_v_bg = sub(J_v_bg_old, scaled(RSJ, dt_f));
        result.J_v_ba = sub(result.J_v_ba, scaled(Delta_R_mid, dt_f));
        result.J_p_bg = sub(add(result.J_p_bg, scaled(J_v_bg_old, dt_f)), scaled(scaled(scaled(RSJ, 0.5f), dt_f), dt_f));
        result.J_p_ba = sub(add(result.J_p_ba, scaled(J_v_ba_old, dt_f)), scaled(scaled(scaled(Delta_R_mid, 0.5f), dt_f), dt_f));

        // --- 15x15 covariance: Sigma <- sym(F Sigma F^T + G Qd G^T); order [dp, dphi, dv, dba, dbg]
        const bool has_noise = params.gyro_noise_density > 0.0f || params.accel_noise_density > 0.0f ||
                               params.gyro_bias_rw_density > 0.0f || params.accel_bias_rw_density > 0.0f;
        bool cov_is_zero = true;  // Eigen's isZero(): every |entry| <= its default precision for float, 1e-5
        for (int i = 0; i < 15 && cov_is_zero; ++i)
            for (int j = 0; j < 15; ++j)
                if (!(fabsf(result.cov[i][j]) <= 1e-5f)) {
                    cov_is_zero = false;
                    break;
                }
        if (has_noise || !cov_is_zero) {
            static thread_local float F[15][15], T[15][15], Q[15][15], G[15][12], GQ[15][12];
            for (int i = 0; i < 15; ++i)
                for (int j = 0; j < 15; ++j) {
                    F[i][j] = (i == j) ? 1.0f : 0.0f;
                    Q[i][j] = 0.0f;
                }
            const M3 R_world_mid = mul(R_world_body_at_reset, Delta_R_mid);
            const M3 gyro_bias_to_mid = scaled(Jr_half, -(0.5f * dt_f));
            const M3 RS = mul(R_world_mid, skew_a);
            const M3 RS_rot = mul(RS, R_half_t), RS_bg = mul(RS, gyro_bias_to_mid);
            set_block(F, 0, 3, scaled(scaled(scaled(RS_rot, -0.5f), dt_f), dt_f));
            set_block(F, 0, 6, scaled(identity3(), dt_f));
            set_block(F, 0, 9, scaled(scaled(scaled(R_world_mid, -0.5f), dt_f), dt_f));
            set_block(F, 0, 12, scaled(scaled(scaled(RS_bg, -0.5f), dt_f), dt_f));
            set_block(F, 3, 3, transposed(R_step));
            set_block(F, 3, 12, scaled(Jr, -dt_f));
            set_block(F, 6, 3, scaled(RS_rot, -dt_f));
            set_block(F, 6, 9, scaled(R_world_mid, -dt_f));
            set_block(F, 6, 12, scaled(RS_bg, -dt_f));
            if (has_noise) {
                const float dt2 = dt_f * dt_f, dt3 = dt2 * dt_f;
                const float sa2 = params.accel_noise_density * params.accel_noise_density;
                const float sg2 = params.gyro_noise_density * params.gyro_noise_density;
                const float sba2 = params.accel_bias_rw_density * params.accel_bias_rw_density;
                const float sbg2 = params.gyro_bias_rw_density * params.gyro_bias_rw_density;
                for (int i = 0; i < 15; ++i)
                    for (int k = 0; k < 12; ++k) G[i][k] = 0.0f;
                const M3 RSJh = mul(RS, Jr_half);
                auto put = [&](int r0, int c0, const M3& B) {
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) G[r0 + i][c0 + j] = B.m[i][j];
                };
                put(0, 0, scaled(R_world_mid, -0.5f * dt2));
                put(6, 0, scaled(R_world_mid, -dt_f));
                put(3, 3, scaled(Jr, -dt_f));
                put(0, 3, scaled(RSJh, 0.25f * dt3));
                put(6, 3, scaled(RSJh, 0.5f * dt2));
                put(9, 6, identity3());
                put(12, 9, identity3());
                const float qd[4] = {sa2 / dt_f, sg2 / dt_f, sba2 * dt_f, sbg2 * dt_f};  // Qd is diagonal
                for (int i = 0; i < 15; ++i)
                    for (int k = 0; k < 12; ++k) GQ[i][k] = G[i][k] * qd[k / 3];
                for (int i = 0; i < 15; ++i)
                    for (int j = 0; j < 15; ++j) {
                        float s = 0.0f;
                        for (int k = 0; k < 12; ++k) s += GQ[i][k] * G[j][k];
                        Q[i][j] = s;
                    }
            }
            for (int i = 0; i < 15; ++i)  // T = F Sigma
                for (int j = 0; j < 15; ++j) {
                    float s = 0.0f;
                    for (int k = 0; k < 15; ++k) s += F[i][k] * result.cov[k][j];
                    T[i][j] = s;
                }
            for (int i = 0; i < 15; ++i)  // Q <- T F^T + Q
                for (int j = 0; j < 15; ++j) {
                    float s = 0.0f;
                    for (int k = 0; k < 15; ++k) s += T[i][k] * F[j][k];
                    Q[i][j] = s + Q[i][j];
                }
            for (int i = 0; i < 15; ++i)  // ensure_symmetric<15> (eigen_utils.hpp:209-219)
                for (int j = 0; j < 15; ++j) result.cov[i][j] = (i == j) ? Q[i][j] : (Q[i][j] + Q[j][i]) * 0.5f;
        }

        ++step_count;
        if (step_count % 100 == 0) {  // back onto SO(3)
            float q[4];
            rot_to_quat(result.Delta_R.m, q);
            quat_to_rot(q, result.Delta_R.m);
        }
    }

    State corrected(const float* bias6) const {  // get_corrected (:244-269)
        float d_bg[3], d_ba[3], phi_corr[3];
        for (int k = 0; k < 3; ++k) {
            d_bg[k] = bias6[k] - bias_gyro[k];
            d_ba[k] = bias6[3 + k] - bias_accel[k];
        }
        State c = result;
        mulv(result.J_R_bg, d_bg, phi_corr);
        c.Delta_R = mul(c.Delta_R, rotation_of(phi_corr));
        // the quaternion round trip: rotation_matrix_to_quaternion, normalize<4>, quaternion_to_rotation_matrix
        float q[4];
        rot_to_quat(c.Delta_R.m, q);
        const float n = sqrtf(fmaf(q[3], q[3], fmaf(q[2], q[2], fmaf(q[1], q[1], fmaf(q[0], q[0], 0.0f)))));
        const float inv = 1.0f / n;
        for (int k = 0; k < 4; ++k) q[k] = (n < 1e-6f) ? 0.0f : q[k] * inv;
        quat_to_rot(q, c.Delta_R.m);
        float vg[3], va[3], pg[3], pa[3];
        mulv(result.J_v_bg, d_bg, vg);
        mulv(result.J_v_ba, d_ba, va);
        mulv(result.J_p_bg, d_bg, pg);
        mulv(result.J_p_ba, d_ba, pa);
        for (int k = 0; k < 3; ++k) {
            c.Delta_v[k] += vg[k] + va[k];
            c.Delta_p[k] += pg[k] + pa[k];
        }
        return c;
    }

    // predict_relative_transform (:307-330): T_body_i -> body_j with gravity and the initial velocity compensated
    Rigid predict_relative(const M3& R_world_body_i, const float v_world_i[3], const float* bias6) const {
        const State c = corrected(bias6);
        const float dt_f = static_cast<float>(c.dt_total);
        const M3 Rt = transposed(R_world_body_i);
        float Rtg[3], Rtv[3];
        mulv(Rt, params.gravity, Rtg);
        mulv(Rt, v_world_i, Rtv);
        Rigid T;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T.R[i][j] = c.Delta_R.m[i][j];
            const float grav_free = c.Delta_p[i] + 0.5f * Rtg[i] * dt_f * dt_f;
            T.t[i] = grav_free + Rtv[i] * dt_f;
        }
        return T;
    }

    Rigid predict(const Rigid& T_world_body_i, const float v_world_i[3], const float* bias6) const {  // :280-295
        const State c = corrected(bias6);
        const float dt_f = static_cast<float>(c.dt_total);
        M3 R_i;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R_i.m[i][j] = T_world_body_i.R[i][j];
        const M3 R_j = mul(R_i, c.Delta_R);
        float Rp[3];
        mulv(R_i, c.Delta_p, Rp);
        Rigid T;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T.R[i][j] = R_j.m[i][j];
            T.t[i] = T_world_body_i.t[i] + v_world_i[i] * dt_f + 0.5f * params.gravity[i] * dt_f * dt_f + Rp[i];
        }
        return T;
    }
};

void export_state(const State& s, sp_imu_state* out) {
    std::memset(out, 0, sizeof(*out));
    store_colmajor3(s.Delta_R, out->Delta_R);
    for (int k = 0; k < 3; ++k) {
        out->Delta_v[k] = s.Delta_v[k];
        out->Delta_p[k] = s.Delta_p[k];
    }
    out->dt_total = s.dt_total;
    store_colmajor3(s.J_R_bg, out->J_R_bg);
    store_colmajor3(s.J_v_bg, out->J_v_bg);
    store_colmajor3(s.J_v_ba, out->J_v_ba);
    store_colmajor3(s.J_p_bg, out->J_p_bg);
    store_colmajor3(s.J_p_ba, out->J_p_ba);
    for (int i = 0; i < 15; ++i)
        for (int j = 0; j < 15; ++j) out->covariance[j * 15 + i] = s.cov[i][j];
}

int invalid(const char* msg) {
    sp_set_error(msg);
    return SP_ERR_INVALID_ARGUMENT;
}

}  // namespace
}  // namespace sp

using sp::Preint;

extern "C" int sp_imu_preint_create(const sp_imu_params* params, void** handle_out) {
    if (!params || !handle_out) return sp::invalid("[sp_imu_preint_create] null params / handle_out");
    Preint* h = new (std::nothrow) Preint();
    if (!h) {
        sp_set_error("[sp_imu_preint_create] out of memory");
        return SP_ERR_RUNTIME;
    }
    h->params = *params;
    *handle_out = h;
    return SP_OK;
}

extern "C" void sp_imu_preint_destroy(void* handle) { delete static_cast<Preint*>(handle); }

extern "C" int sp_imu_preint_reset(void* handle, const float* bias6_host, const float* covariance225_host,
                                   const float* R_world_body9_host) {
    if (!handle) return sp::invalid("[sp_imu_preint_reset] null handle");
    static_cast<Preint*>(handle)->reset(bias6_host, covariance225_host, R_world_body9_host);
    return SP_OK;
}

extern "C" int sp_imu_preint_integrate(void* handle, double timestamp, const float* gyro3_host, const float* accel3_host) {
    if (!handle || !gyro3_host || !accel3_host) return sp::invalid("[sp_imu_preint_integrate] null handle / gyro / accel");
    sp::Sample s;
    s.timestamp = timestamp;
    for (int k = 0; k < 3; ++k) {
        s.gyro[k] = gyro3_host[k];
        s.accel[k] = accel3_host[k];
    }
    static_cast<Preint*>(handle)->integrate(s);
    return SP_OK;
}

extern "C" int sp_imu_preint_num_measurements(void* handle) { return handle ? static_cast<Preint*>(handle)->num_measurements : 0; }

extern "C" int sp_imu_preint_get(void* handle, const float* bias6_host, sp_imu_state* state_out) {
    if (!handle || !state_out) return sp::invalid("[sp_imu_preint_get] null handle / state_out");
    const Preint* h = static_cast<Preint*>(handle);
    if (bias6_host)
        sp::export_state(h->corrected(bias6_host), state_out);
    else
        sp::export_state(h->result, state_out);
    return SP_OK;
}

extern "C" int sp_imu_preint_predict_relative(void* handle, const float* R_world_body9_host, const float* v_world3_host,
                                              const float* bias6_host, float* T16_out_host) {
    if (!handle || !R_world_body9_host || !v_world3_host || !bias6_host || !T16_out_host)
        return sp::invalid("[sp_imu_preint_predict_relative] null argument");
    sp::store_rigid_colmajor(static_cast<Preint*>(handle)->predict_relative(sp::load_colmajor3(R_world_body9_host), v_world3_host, bias6_host),
                             T16_out_host);
    return SP_OK;
}

extern "C" int sp_imu_preint_predict_transform(void* handle, const float* T_world_body16_host, const float* v_world3_host,
                                               const float* bias6_host, float* T16_out_host) {
    if (!handle || !T_world_body16_host || !v_world3_host || !bias6_host || !T16_out_host)
        return sp::invalid("[sp_imu_preint_predict_transform] null argument");
    sp::store_rigid_colmajor(static_cast<Preint*>(handle)->predict(sp::load_rigid_colmajor(T_world_body16_host), v_world3_host, bias6_host),
                             T16_out_host);
    return SP_OK;
}

extern "C" int sp_imu_deskew_trajectory_host(const double* stamps_host, const float* gyro_accel_host, size_t n,
                                             double scan_start_sec, double scan_duration_sec, const float* T_imu_to_lidar16_host,
                                             const float* bias6_host, const sp_imu_params* params,
                                             const float* R_world_body9_host, const float* v_world3_host, int gyro_only,
                                             float* traj_out_host, size_t capacity, size_t* n_traj_out, int* status_out) {
    using namespace sp;
    if ((n > 0 && (!stamps_host || !gyro_accel_host)) || !T_imu_to_lidar16_host || !bias6_host || !params || !R_world_body9_host ||
        !v_world3_host || !traj_out_host || !n_traj_out || !status_out)
        return invalid("[sp_imu_deskew_trajectory_host] null argument");
    *n_traj_out = 0;
    if (scan_duration_sec <= 0.0) {  // imu_deskew.hpp:151-155
        *status_out = SP_IMU_DESKEW_INVALID_SCAN_DURATION;
        return SP_OK;
    }
    const double scan_end_sec = scan_start_sec + scan_duration_sec;
    // step 1 (:161-179): the samples of the scan window and a 50 ms margin on either side
    constexpr double kMarginSec = 0.05;
    std::vector<Sample> filtered;
    filtered.reserve(256);
    for (size_t i = 0; i < n; ++i)
        if (stamps_host[i] >= scan_start_sec - kMarginSec && stamps_host[i] <= scan_end_sec + kMarginSec) {
            Sample s;
            s.timestamp = stamps_host[i];
            for (int k = 0; k < 3; ++k) {
                s.gyro[k] = gyro_accel_host[6 * i + k];
                s.accel[k] = gyro_accel_host[6 * i + 3 + k];
            }
            filtered.push_back(s);
        }
    *status_out = SP_IMU_DESKEW_INSUFFICIENT_IMU_COVERAGE;
    if (filtered.size() < 2) return SP_OK;
    if (filtered.front().timestamp > scan_start_sec + kMarginSec || filtered.back().timestamp < scan_end_sec - kMarginSec) return SP_OK;
    // step 2 (:185-214): a virtual sample at exactly scan_start_sec
    Sample m_start;
    m_start.timestamp = scan_start_sec;
    auto it_next = std::lower_bound(filtered.begin(), filtered.end(), scan_start_sec,
                                    [](const Sample& m, double t) { return m.timestamp < t; });
    if (it_next == filtered.begin()) {
        m_start = *it_next;
        m_start.timestamp = scan_start_sec;
    } else if (it_next == filtered.end()) {
        m_start = filtered.back();
        m_start.timestamp = scan_start_sec;
    } else {
        const Sample& prev_m = *(it_next - 1);
        const float alpha = static_cast<float>((scan_start_sec - prev_m.timestamp) / (it_next->timestamp - prev_m.timestamp));
        for (int k = 0; k < 3; ++k) {
            m_start.gyro[k] = std::fma(it_next->gyro[k] - prev_m.gyro[k], alpha, prev_m.gyro[k]);
            m_start.accel[k] = std::fma(it_next->accel[k] - prev_m.accel[k], alpha, prev_m.accel[k]);
        }
    }
    // step 3 (:221-285): the LiDAR-frame pose relative to scan start at every sample from scan start on
    if (capacity < 1) return invalid("[sp_imu_deskew_trajectory_host] capacity is smaller than the trajectory (n + 1 always suffices)");
    size_t m = 0;
    auto push = [&](const float q[4], const float t[3], float stamp) {
        float* e = traj_out_host + 8 * m++;
        for (int k = 0; k < 4; ++k) e[k] = q[k];
        for (int k = 0; k < 3; ++k) e[4 + k] = t[k];
        e[7] = stamp;
    };
    const float q_id[4] = {0.0f, 0.0f, 0.0f, 1.0f}, t_zero[3] = {0.0f, 0.0f, 0.0f};
    push(q_id, t_zero, 0.0f);
    Preint integ;
    integ.params = *params;
    integ.reset(bias6_host, nullptr, nullptr);
    integ.integrate(m_start);
    const Rigid T_il = load_rigid_colmajor(T_imu_to_lidar16_host);
    const Rigid T_il_inv = rigid_inverse(T_il);
    const M3 R_wb = load_colmajor3(R_world_body9_host);
    for (auto it = it_next; it != filtered.end(); ++it) {
        if (it->timestamp > scan_end_sec + kMarginSec) break;
        integ.integrate(*it);
        const float t_rel_sec = static_cast<float>(it->timestamp - scan_start_sec);
        if (t_rel_sec < 0.0f) continue;
        Rigid T_imu_rel;
        if (gyro_only) {  // rotation only: neither the velocity nor the integrated acceleration moves a point
            const State c = integ.corrected(bias6_host);
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) T_imu_rel.R[i][j] = c.Delta_R.m[i][j];
                T_imu_rel.t[i] = 0.0f;
            }
        } else {
            T_imu_rel = integ.predict_relative(R_wb, v_world3_host, bias6_host);
        }
        const Rigid T_lidar_rel = rigid_mul(rigid_mul(T_il, T_imu_rel), T_il_inv);
        float q[4];
        rot_to_quat(T_lidar_rel.R, q);  // the project's conversion where the reference uses Eigen::Quaternionf's
        if (m >= capacity) return invalid("[sp_imu_deskew_trajectory_host] capacity is smaller than the trajectory (n + 1 always suffices)");
        push(q, T_lidar_rel.t, t_rel_sec);
    }
    if (m < 2) return SP_OK;
    if (traj_out_host[8 * (m - 1) + 7] < static_cast<float>(scan_duration_sec) - static_cast<float>(kMarginSec)) return SP_OK;
    *n_traj_out = m;
    *status_out = SP_IMU_DESKEW_SUCCESS;
    return SP_OK;
}

extern "C" int sp_imu_deskew_intervals_host(const float* traj_host, size_t n_traj, float* intervals_out_host) {
    using namespace sp;
    if (!traj_host || !intervals_out_host || n_traj < 2)
        return invalid("[sp_imu_deskew_intervals_host] null traj / intervals_out, or fewer than two poses");
    for (size_t i = 0; i + 1 < n_traj; ++i) {
        const float *e0 = traj_host + 8 * i, *e1 = e0 + 8;
        float* row = intervals_out_host + 16 * i;
        // quat_slerp's first half (imu_deskew.hpp:54-73): the shorter arc, conj(q0) * q1, so3_log
        float q1[4] = {e1[0], e1[1], e1[2], e1[3]};
        const float d = fmaf(e0[3], q1[3], fmaf(e0[2], q1[2], fmaf(e0[1], q1[1], fmaf(e0[0], q1[0], 0.0f))));  // dot<4>
        if (d < 0.0f)
            for (int k = 0; k < 4; ++k) q1[k] *= -1.0f;
        const float q0_conj[4] = {-e0[0], -e0[1], -e0[2], e0[3]};
        float delta_q[4], omega[3];
        quat_mult(q0_conj, q1, delta_q);
        so3_log(delta_q, omega);
        row[0] = e0[7];
        row[1] = e1[7];
        for (int k = 0; k < 4; ++k) row[2 + k] = e0[k];
        for (int k = 0; k < 3; ++k) {
            row[6 + k] = omega[k];
            row[9 + k] = e0[4 + k];
            row[12 + k] = e1[4 + k] - e0[4 + k];
        }
        row[15] = 0.0f;
    }
    return SP_OK;
}
