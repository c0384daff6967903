// Host numerics and control flow of the tightly coupled LiDAR-inertial alignment: the IMU prior factor (imu_factor.hpp = A), the
// 15x15 algebra of lio_registration.hpp (= B) and LIORegistration::align (B:396-648) as a state machine in the shape of
// sp_opt_stepper_*: the caller linearises and evaluates trials with the kernels Registration already has, everything else is
// decided here; and what the per-frame loop of pipeline/lidar_inertial_odometry.hpp (= L) computes between its stages (the bias
// observability test, the bias clamp, the state prediction, the covariance handed to the next IMU window).
// Plain host arithmetic (the reference runs all of it on the host with Eigen); no kernel is in this file.
// 15x15 matrices are column-major, a state is p3 | R9 column-major | v3 | b_a3 | b_g3.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>

#include "sp_common.h"
#include "sp_math.h"
#include "sp_pose_math.h"
#include "sp_lio_math.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

constexpr int kN = 15, kPos = 0, kRot = 3, kVel = 6, kAcc = 9, kGyr = 12;  // imu::State::kIdx*

struct LioState {
    float p[3];
    float R[3][3];
    float v[3], ba[3], bg[3];
};

LioState load_state(const float* s) {
    LioState x;
    for (int i = 0; i < 3; ++i) {
        x.p[i] = s[i];
        for (int j = 0; j < 3; ++j) x.R[i][j] = s[3 + j * 3 + i];
        x.v[i] = s[12 + i];
        x.ba[i] = s[15 + i];
        x.bg[i] = s[18 + i];
    }
    return x;
}
void store_state(const LioState& x, float* s) {
    for (int i = 0; i < 3; ++i) {
        s[i] = x.p[i];
        for (int j = 0; j < 3; ++j) s[3 + j * 3 + i] = x.R[i][j];
        s[12 + i] = x.v[i];
        s[15 + i] = x.ba[i];
        s[18 + i] = x.bg[i];
    }
}
void state_to_pose(const LioState& x, float* T16) {
    for (int j = 0; j < 3; ++j) {
        for (int i = 0; i < 3; ++i) T16[j * 4 + i] = x.R[i][j];
        T16[j * 4 + 3] = 0.0f;
        T16[12 + j] = x.p[j];
    }
    T16[15] = 1.0f;
}

void mul33(const float A[3][3], const float B[3][3], float out[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 3; ++k) s += A[i][k] * B[k][j];
            out[i][j] = s;
        }
}

// A:71-85
void manifold_residual(const LioState& pred, const LioState& op, float r[kN]) {
    float Rrel[3][3], q[4];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 3; ++k) s += pred.R[k][i] * op.R[k][j];
            Rrel[i][j] = s;
        }
    rot_to_quat(Rrel, q);
    so3_log(q, r + kRot);
    for (int i = 0; i < 3; ++i) {
        r[kPos + i] = op.p[i] - pred.p[i];
        r[kVel + i] = op.v[i] - pred.v[i];
        r[kAcc + i] = op.ba[i] - pred.ba[i];
        r[kGyr + i] = op.bg[i] - pred.bg[i];
    }
}

// A:116-141
bool imu_hessian_gradient(const LioState& pred, const LioState& op, const float* P, float* H, float* b) {
    LdltN ldlt;
    ldlt.compute(P, kN);
    if (!ldlt.positive()) {
        std::memset(H, 0, sizeof(float) * kN * kN);
        std::memset(b, 0, sizeof(float) * kN);
        return false;
    }
    ldlt.inverse(H);
    float r[kN];
    manifold_residual(pred, op, r);
    ldlt.solve(r, b);
    return true;
}

// B:260-273
LioState retract(const LioState& x, const float* d) {
    LioState u = x;
    float q[4], dR[3][3];
    so3_exp(d + kRot, q);
    quat_to_rot(q, dR);
    mul33(x.R, dR, u.R);
    for (int i = 0; i < 3; ++i) {
        u.p[i] += d[kPos + i];
        u.v[i] += d[kVel + i];
        u.ba[i] += d[kAcc + i];
        u.bg[i] += d[kGyr + i];
    }
    return u;
}

inline float& at(float* H, int i, int j) { return H[j * kN + i]; }

// B:94-113; the 6x6 of sp_linearized is row-major, order [d_omega, d_t]
void add_icp_factor(sp_lio_linearized* res, const sp_linearized* icp, const float R[3][3], float weight) {
    auto Hi = [&](int i, int j) { return icp->H[i * 6 + j]; };
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) at(res->H, kRot + i, kRot + j) += weight * Hi(i, j);
        res->b[kRot + i] += weight * icp->b[i];
    }
    float RH[3][3];  // R * H_tt
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 3; ++k) s += R[i][k] * Hi(3 + k, 3 + j);
            RH[i][j] = s;
        }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            float pp = 0.0f, pr = 0.0f, rp = 0.0f;
            for (int k = 0; k < 3; ++k) {
                pp += RH[i][k] * R[j][k];         // (R H_tt) R^T
                pr += R[i][k] * Hi(3 + k, j);     // R H_tw
                rp += Hi(i, 3 + k) * R[j][k];     // H_wt R^T
            }
            at(res->H, kPos + i, kPos + j) += weight * pp;
            at(res->H, kPos + i, kRot + j) += weight * pr;
            at(res->H, kRot + i, kPos + j) += weight * rp;
        }
        float s = 0.0f;
        for (int k = 0; k < 3; ++k) s += R[i][k] * icp->b[3 + k];
        res->b[kPos + i] += weight * s;
    }
    res->error_icp += weight * icp->error;
    res->inlier += icp->inlier;
}

inline float clamp01(float x) { return x < 0.0f ? 0.0f : (1.0f < x ? 1.0f : x); }

// compute_block_filter (B:162-185): sum_i sqrt(scale_i) q_i q_i^T, written as I - sum_i (1 - sqrt(scale_i)) q_i q_i^T. The two are
// equal for orthonormal q_i; eigen_sym3's Jacobi rotations leave them orthonormal to a few float roundings only, and in this form
// that defect enters scaled by (1 - sqrt(scale_i)): a direction that is not weak passes through exactly (F H F = H).
void block_filter(const float Hp[6][6], int o, float min_eig_per_inlier, float weak_direction_scale, uint32_t inlier,
                  float F[6][6]) {
    float blk[3][3], lam[3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) blk[i][j] = Hp[o + i][o + j];
    eigen_sym3(blk, lam, V);  // symmetrises its input
    const float min_info = fmaxf(0.0f, min_eig_per_inlier) * (float)inlier;
    const float weak_scale = clamp01(weak_direction_scale);
    for (int i = 0; i < 3; ++i) F[o + i][o + i] = 1.0f;
    for (int e = 0; e < 3; ++e) {
        const float lambda = fmaxf(0.0f, lam[e]);
        float scale = 1.0f;
        if (lambda <= 0.0f || !(fabsf(lambda) <= FLT_MAX)) scale = 0.0f;
        else if (min_info > 0.0f) scale = fmaxf(weak_scale, clamp01(lambda / min_info));
        const float cut = 1.0f - sqrtf(clamp01(scale));
        if (cut == 0.0f) continue;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) F[o + r][o + c] -= cut * (V[r][e] * V[c][e]);
    }
}

// B:144-202
void directional_weighting(sp_lio_linearized* f, const sp_lio_directional_params& p) {
    if (!p.enable || f->inlier == 0) return;
    static const int map[6] = {kPos, kPos + 1, kPos + 2, kRot, kRot + 1, kRot + 2};
    float Hp[6][6], bp[6], F[6][6] = {};
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) Hp[i][j] = 0.5f * (at(f->H, map[i], map[j]) + at(f->H, map[j], map[i]));
        bp[i] = f->b[map[i]];
    }
    block_filter(Hp, 0, p.trans_min_eigenvalue_per_inlier, p.trans_weak_direction_scale, f->inlier, F);
    block_filter(Hp, 3, p.rot_min_eigenvalue_per_inlier, p.rot_weak_direction_scale, f->inlier, F);
    float FH[6][6], Fb[6];
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 6; ++k) s += F[i][k] * Hp[k][j];
            FH[i][j] = s;
        }
        float s = 0.0f;
        for (int k = 0; k < 6; ++k) s += F[i][k] * bp[k];
        Fb[i] = s;
    }
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 6; ++k) s += FH[i][k] * F[k][j];
            at(f->H, map[i], map[j]) = s;
        }
        float s = 0.0f;
        for (int k = 0; k < 6; ++k) s += F[i][k] * Fb[k];
        f->b[map[i]] = s;
    }
}

// B:224-238
bool solve_ldlt(const float* H, const float* b, float* delta, float* P_post) {
    LdltN ldlt;
    ldlt.compute(H, kN);
    if (!ldlt.positive()) {
        std::memset(delta, 0, sizeof(float) * kN);
        if (P_post) std::memset(P_post, 0, sizeof(float) * kN * kN);
        return false;
    }
    float nb[kN];
    for (int i = 0; i < kN; ++i) nb[i] = -b[i];
    ldlt.solve(nb, delta);
    if (P_post) ldlt.inverse(P_post);
    return true;
}

// the two non-identity blocks of J (B:308-323) or of its analytic inverse (B:366-378)
void extrinsic_blocks(const float* T16, const float* R9, bool inverse, float Brr[3][3], float Bpr[3][3]) {
    const Rigid T = load_rigid_colmajor(T16);
    const Rigid Ti = rigid_inverse(T);
    float Rwl[3][3], Rwi[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rwl[i][j] = R9[j * 3 + i];
    mul33(Rwl, T.R, Rwi);
    const float* t = Ti.t;  // the LiDAR origin in the IMU body frame
    const float S[3][3] = {{0.0f, -t[2], t[1]}, {t[2], 0.0f, -t[0]}, {-t[1], t[0], 0.0f}};
    float RS[3][3];
    mul33(Rwi, S, RS);
    if (!inverse) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) { Brr[i][j] = T.R[i][j]; Bpr[i][j] = -RS[i][j]; }
    } else {
        float Ril[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Ril[i][j] = T.R[j][i];
        mul33(RS, Ril, Bpr);
        std::memcpy(Brr, Ril, sizeof(Ril));
    }
}
void fill_jacobian(const float Brr[3][3], const float Bpr[3][3], float* J) {
    std::memset(J, 0, sizeof(float) * kN * kN);
    for (int i = 0; i < kN; ++i) at(J, i, i) = 1.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            at(J, kRot + i, kRot + j) = Brr[i][j];
            at(J, kPos + i, kRot + j) = Bpr[i][j];
        }
}
// J P J^T (B:340-345) or J^-1 P J^-T (B:366-381); P_out is not P
void transform_covariance(const float* P, const float* T16, const float* R9, bool lidar_to_imu, float* P_out) {
    float Brr[3][3], Bpr[3][3], J[225], JP[225];
    extrinsic_blocks(T16, R9, lidar_to_imu, Brr, Bpr);
    fill_jacobian(Brr, Bpr, J);
    for (int i = 0; i < kN; ++i)
        for (int j = 0; j < kN; ++j) {
            float s = 0.0f;
            for (int k = 0; k < kN; ++k) s += J[k * kN + i] * P[j * kN + k];
            JP[j * kN + i] = s;
        }
    for (int i = 0; i < kN; ++i)
        for (int j = 0; j < kN; ++j) {
            float s = 0.0f;
            for (int k = 0; k < kN; ++k) s += JP[k * kN + i] * J[k * kN + j];
            P_out[j * kN + i] = s;
        }
}

}  // namespace
}  // namespace sp

// ------------------------------------------------------------------------------------------------ the state machine
enum { LIO_PHASE_LIN = 0, LIO_PHASE_TRIAL_CURRENT = 1, LIO_PHASE_TRIAL_CANDIDATE = 2 };

struct sp_lio_stepper {
    sp_lio_params prm;
    sp_lio_factor_facts facts;
    int update_bias;
    sp::LioState pred, op, trial_state, lin_state;
    float P_prev[225];
    float H_imu[225], b_imu[15];
    bool imu_valid;
    // schedule (B:443-476)
    int levels, base_iterations, extra_iterations;
    float robust_scale, rotation_robust_scale, robust_factor, rotation_robust_factor;
    // loop
    int done, phase, level, solver_iter, solver_iterations;
    uint32_t actual_iterations;
    float lm_lambda, radius;
    float icp_weight, current_cost;
    int inner;
    float trial_delta[15];
    float dogleg_step_norm, predicted_reduction;
    sp_lio_linearized lio;  // the combined system of the latest linearisation, undamped
    float last_error;
    uint32_t last_inlier;
    float H_undamped[225];
    bool has_H_undamped;
};

namespace sp {
namespace {

float clampf(float x, float lo, float hi) { return x < lo ? lo : (hi < x ? hi : x); }  // std::clamp

float imu_cost(const sp_lio_stepper& s, const LioState& x) {  // B:430-434
    if (!s.imu_valid) return 0.0f;
    float r[kN], Hr[kN];
    manifold_residual(s.pred, x, r);
    matvec_n(s.H_imu, r, Hr, kN);
    return 0.5f * dot_n(r, Hr, kN);
}
void bias_freeze(const sp_lio_stepper& s, float* d) {  // B:436-441
    if (!s.update_bias)
        for (int i = 0; i < 6; ++i) d[kAcc + i] = 0.0f;
}
bool solve_damped(const sp_lio_stepper& s, float lambda, float* delta) {
    float Hd[225];
    std::memcpy(Hd, s.lio.H, sizeof(Hd));
    for (int i = 0; i < kN; ++i) at(Hd, i, i) += lambda;
    return solve_ldlt(Hd, s.lio.b, delta, nullptr);
}
float clamp_radius(const sp_lio_stepper& s, float r) { return clampf(r, s.prm.opt.dl_min_radius, s.prm.opt.dl_max_radius); }
float clamp_lambda(const sp_lio_stepper& s, float l) { return clampf(l, s.prm.opt.lm_min_lambda, s.prm.opt.lm_max_lambda); }

void begin_level(sp_lio_stepper& s) {  // B:484-486
    s.lm_lambda = s.prm.opt.lm_init_lambda;
    s.radius = s.prm.opt.dl_initial_radius;
    s.solver_iterations = s.base_iterations + (s.level < s.extra_iterations ? 1 : 0);
    s.solver_iter = 0;
    s.phase = LIO_PHASE_LIN;
}
void end_level(sp_lio_stepper& s) {  // B:635-636
    if (s.level + 1 >= s.levels) { s.done = 1; return; }  // (the scales of the last level stay: a DONE request reports them)
    s.robust_scale *= s.robust_factor;
    s.rotation_robust_scale *= s.rotation_robust_factor;
    ++s.level;
    begin_level(s);
}
// B:625-632
void end_iteration(sp_lio_stepper& s, bool accepted, bool stop, const float* delta) {
    std::memcpy(s.H_undamped, s.lio.H, sizeof(s.H_undamped));
    s.has_H_undamped = true;
    if (accepted) {
        s.op = retract(s.op, delta);
        const float dr = sqrtf(dot_n(delta + kRot, delta + kRot, 3)), dt = sqrtf(dot_n(delta + kPos, delta + kPos, 3));
        if (dr < s.prm.opt.crit_rotation && dt < s.prm.opt.crit_translation) { end_level(s); return; }
    } else if (stop) {
        end_level(s);
        return;
    }
    if (++s.solver_iter >= s.solver_iterations) { end_level(s); return; }
    s.phase = LIO_PHASE_LIN;
}
// the next LM trial that can be formed (B:552-581), or the end of the level when there is none
void lm_next_trial(sp_lio_stepper& s) {
    for (; s.inner < s.prm.opt.lm_max_inner_iterations; ++s.inner) {
        if (solve_damped(s, s.lm_lambda, s.trial_delta)) {
            bias_freeze(s, s.trial_delta);
            s.trial_state = retract(s.op, s.trial_delta);
            s.phase = LIO_PHASE_TRIAL_CANDIDATE;
            return;
        }
        s.lm_lambda = clamp_lambda(s, s.lm_lambda * s.prm.opt.lm_lambda_factor);
    }
    end_iteration(s, false, true, nullptr);
}

}  // namespace
}  // namespace sp

extern "C" int sp_imu_manifold_residual_host(const float* x_pred21, const float* x_op21, float* r15_out) {
    if (!x_pred21 || !x_op21 || !r15_out) return SP_ERR_INVALID_ARGUMENT;
    sp::manifold_residual(sp::load_state(x_pred21), sp::load_state(x_op21), r15_out);
    return SP_OK;
}

extern "C" int sp_imu_hessian_gradient_host(const float* x_pred21, const float* x_op21, const float* P225, float* H225_out,
                                            float* b15_out, int* valid_out) {
    if (!x_pred21 || !x_op21 || !P225 || !H225_out || !b15_out || !valid_out) return SP_ERR_INVALID_ARGUMENT;
    *valid_out = sp::imu_hessian_gradient(sp::load_state(x_pred21), sp::load_state(x_op21), P225, H225_out, b15_out) ? 1 : 0;
    return SP_OK;
}

extern "C" int sp_imu_gradient_host(const float* x_pred21, const float* x_op21, const float* H225, float* b15_out) {
    if (!x_pred21 || !x_op21 || !H225 || !b15_out) return SP_ERR_INVALID_ARGUMENT;
    float r[15];
    sp::manifold_residual(sp::load_state(x_pred21), sp::load_state(x_op21), r);
    sp::matvec_n(H225, r, b15_out, 15);
    return SP_OK;
}

extern "C" int sp_lio_add_icp_factor_host(sp_lio_linearized* result, const sp_linearized* icp, const float* R_world_lidar9,
                                          float weight) {
    if (!result || !icp || !R_world_lidar9) return SP_ERR_INVALID_ARGUMENT;
    float R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = R_world_lidar9[j * 3 + i];
    sp::add_icp_factor(result, icp, R, weight);
    return SP_OK;
}

extern "C" int sp_lio_directional_weighting_host(sp_lio_linearized* icp_factor, const sp_lio_directional_params* params) {
    if (!icp_factor || !params) return SP_ERR_INVALID_ARGUMENT;
    sp::directional_weighting(icp_factor, *params);
    return SP_OK;
}

extern "C" int sp_lio_solve_ldlt_host(const float* H225, const float* b15, float* delta15_out, float* P_post225_opt, int* ok_out) {
    if (!H225 || !b15 || !delta15_out || !ok_out) return SP_ERR_INVALID_ARGUMENT;
    *ok_out = sp::solve_ldlt(H225, b15, delta15_out, P_post225_opt) ? 1 : 0;
    return SP_OK;
}

extern "C" int sp_lio_retract_host(const float* x21, const float* delta15, float* x_out21) {
    if (!x21 || !delta15 || !x_out21) return SP_ERR_INVALID_ARGUMENT;
    sp::store_state(sp::retract(sp::load_state(x21), delta15), x_out21);
    return SP_OK;
}

extern "C" int sp_lio_imu_to_lidar_jacobian_host(const float* T_imu_to_lidar16, const float* R_world_lidar9, float* J225_out) {
    if (!T_imu_to_lidar16 || !R_world_lidar9 || !J225_out) return SP_ERR_INVALID_ARGUMENT;
    float Brr[3][3], Bpr[3][3];
    sp::extrinsic_blocks(T_imu_to_lidar16, R_world_lidar9, false, Brr, Bpr);
    sp::fill_jacobian(Brr, Bpr, J225_out);
    return SP_OK;
}

extern "C" int sp_lio_transform_covariance_host(const float* P225, const float* T_imu_to_lidar16, const float* R_world_lidar9,
                                                int lidar_to_imu, float* P_out225) {
    if (!P225 || !T_imu_to_lidar16 || !R_world_lidar9 || !P_out225 || P225 == P_out225) return SP_ERR_INVALID_ARGUMENT;
    sp::transform_covariance(P225, T_imu_to_lidar16, R_world_lidar9, lidar_to_imu != 0, P_out225);
    return SP_OK;
}

// ------------------------------------------------------------------------------------------------ the per-frame LIO loop
// What LidarInertialOdometryPipeline (pipeline/lidar_inertial_odometry.hpp = L) computes and decides between its stages.

extern "C" int sp_lio_bias_observable_host(const float* gyro_host, const float* accel_host, size_t n, int freeze_on_low_excitation,
                                           float gyro_excitation_threshold, float accel_excitation_threshold, int* observable_out) {
    if (!observable_out) return SP_ERR_INVALID_ARGUMENT;
    if (!freeze_on_low_excitation) { *observable_out = 1; return SP_OK; }  // L:373
    if (n < 2) { *observable_out = 0; return SP_OK; }                       // L:374
    if (!gyro_host || !accel_host) return SP_ERR_INVALID_ARGUMENT;
    float gyro_mean[3] = {0.0f, 0.0f, 0.0f}, accel_mean[3] = {0.0f, 0.0f, 0.0f};
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            gyro_mean[k] += gyro_host[3 * i + k];
            accel_mean[k] += accel_host[3 * i + k];
        }
    const float count = (float)n;
    for (int k = 0; k < 3; ++k) {
        gyro_mean[k] /= count;
        accel_mean[k] /= count;
    }
    float gyro_dev = 0.0f, accel_dev = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        float dg[3], da[3];
        for (int k = 0; k < 3; ++k) {
            dg[k] = gyro_host[3 * i + k] - gyro_mean[k];
            da[k] = accel_host[3 * i + k] - accel_mean[k];
        }
        gyro_dev = fmaxf(gyro_dev, sqrtf(sp::dot_n(dg, dg, 3)));
        accel_dev = fmaxf(accel_dev, sqrtf(sp::dot_n(da, da, 3)));
    }
    *observable_out = (gyro_dev > gyro_excitation_threshold || accel_dev > accel_excitation_threshold) ? 1 : 0;
    return SP_OK;
}

extern "C" int sp_lio_clamp_bias_host(float* bias3, float max_norm) {
    if (!bias3) return SP_ERR_INVALID_ARGUMENT;
    if (max_norm <= 0.0f) return SP_OK;
    const float norm = sqrtf(sp::dot_n(bias3, bias3, 3));
    if (norm > max_norm) {
        const float scale = max_norm / norm;
        for (int k = 0; k < 3; ++k) bias3[k] *= scale;
    }
    return SP_OK;
}

extern "C" int sp_lio_predict_state_host(const float* x21, const float* T_imu_to_lidar16, const float* T_imu_rel16,
                                         const float* Delta_v3, float dt_total, const float* gravity3, float* x_pred_out21) {
    if (!x21 || !T_imu_to_lidar16 || !T_imu_rel16 || !Delta_v3 || !gravity3 || !x_pred_out21) return SP_ERR_INVALID_ARGUMENT;
    using namespace sp;
    const LioState x = load_state(x21);
    const Rigid T_i2l = load_rigid_colmajor(T_imu_to_lidar16);
    // T_lidar_rel = T_i2l * T_imu_rel * T_i2l^-1, T_pred = pose(x) * T_lidar_rel (L:443-445)
    const Rigid T_lidar_rel = rigid_mul(rigid_mul(T_i2l, load_rigid_colmajor(T_imu_rel16)), rigid_inverse(T_i2l));
    Rigid pose;
    std::memcpy(pose.R, x.R, sizeof(pose.R));
    std::memcpy(pose.t, x.p, sizeof(pose.t));
    const Rigid T_pred = rigid_mul(pose, T_lidar_rel);
    LioState pred = x;  // the biases are copied (L:456-457)
    std::memcpy(pred.R, T_pred.R, sizeof(pred.R));
    std::memcpy(pred.p, T_pred.t, sizeof(pred.p));
    float R_world_imu[3][3];
    mul33(x.R, T_i2l.R, R_world_imu);
    for (int i = 0; i < 3; ++i) {  // v + g dt + R_world_imu Delta_v (L:455)
        float s = 0.0f;
        for (int k = 0; k < 3; ++k) s += R_world_imu[i][k] * Delta_v3[k];
        pred.v[i] = (x.v[i] + gravity3[i] * dt_total) + s;
    }
    store_state(pred, x_pred_out21);
    return SP_OK;
}

extern "C" int sp_lio_reset_covariance_host(const float* P_post225, float fd_velocity_sigma, float icp_rotation_sigma,
                                            const float* T_imu_to_lidar16, const float* R_world_lidar9, float* P_initial_imu225_out,
                                            float* R_world_imu9_out) {
    if (!P_post225 || !T_imu_to_lidar16 || !R_world_lidar9 || !P_initial_imu225_out || !R_world_imu9_out ||
        P_post225 == P_initial_imu225_out)
        return SP_ERR_INVALID_ARGUMENT;
    using namespace sp;
    float P_initial[225];
    std::memcpy(P_initial, P_post225, sizeof(P_initial));
    const float sv2 = fd_velocity_sigma * fd_velocity_sigma, sr2 = icp_rotation_sigma * icp_rotation_sigma;
    for (int i = 0; i < 3; ++i) {  // the floors (L:412-417)
        at(P_initial, kVel + i, kVel + i) += sv2;
        at(P_initial, kRot + i, kRot + i) += sr2;
    }
    transform_covariance(P_initial, T_imu_to_lidar16, R_world_lidar9, true, P_initial_imu225_out);  // L:423-424
    const Rigid T_i2l = load_rigid_colmajor(T_imu_to_lidar16);
    float Rwl[3][3], Rwi[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rwl[i][j] = R_world_lidar9[j * 3 + i];
    mul33(Rwl, T_i2l.R, Rwi);  // L:404
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R_world_imu9_out[j * 3 + i] = Rwi[i][j];
    return SP_OK;
}

extern "C" int sp_dogleg_step_n_host(int n, const float* H, const float* g, float trust_region_radius, float* p_out,
                                     float* step_norm_out, float* predicted_reduction_out) {
    if (n != 6 && n != 15) {
        sp_set_error("[sp_dogleg_step_n_host] n must be 6 or 15");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (!H || !g || !p_out || !step_norm_out || !predicted_reduction_out) return SP_ERR_INVALID_ARGUMENT;
    const sp::DoglegStepN r = sp::dogleg_step_n(H, g, trust_region_radius, n);
    for (int i = 0; i < n; ++i) p_out[i] = r.p[i];
    *step_norm_out = r.step_norm;
    *predicted_reduction_out = r.predicted_reduction;
    return SP_OK;
}

extern "C" int sp_lio_stepper_create(const sp_lio_params* params, const sp_lio_factor_facts* facts, const float* predicted_state21,
                                     const float* predicted_covariance225, const float* previous_posterior_covariance225,
                                     int update_bias, sp_lio_stepper** out) {
    if (!params || !facts || !predicted_state21 || !predicted_covariance225 || !previous_posterior_covariance225 || !out)
        return SP_ERR_INVALID_ARGUMENT;
    const sp_opt_params& o = params->opt;
    if (o.method != SP_OPT_GAUSS_NEWTON && o.method != SP_OPT_LEVENBERG_MARQUARDT && o.method != SP_OPT_POWELL_DOGLEG) {
        sp_set_error("[sp_lio_stepper_create] unknown optimization method");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (o.max_iterations < 0 || o.lm_max_inner_iterations < 0 || params->robust_auto_scaling_iter < 0) {
        sp_set_error("[sp_lio_stepper_create] iteration counts must not be negative");
        return SP_ERR_INVALID_ARGUMENT;
    }
    if (facts->residual_dim != 1 && facts->residual_dim != 3) {
        sp_set_error("[sp_lio_stepper_create] residual_dim must be 1 or 3");
        return SP_ERR_INVALID_ARGUMENT;
    }
    sp_lio_stepper* const s = new (std::nothrow) sp_lio_stepper();  // (zeroed)
    if (!s) return SP_ERR_RUNTIME;
    s->prm = *params;
    s->facts = *facts;
    s->update_bias = update_bias;
    s->pred = s->op = s->trial_state = s->lin_state = sp::load_state(predicted_state21);
    std::memcpy(s->P_prev, previous_posterior_covariance225, sizeof(s->P_prev));
    s->imu_valid = sp::imu_hessian_gradient(s->pred, s->pred, predicted_covariance225, s->H_imu, s->b_imu);  // B:401-404
    s->icp_weight = 1.0f;
    s->last_error = FLT_MAX;  // LinearizedResult's defaults
    s->last_inlier = 0;

    // B:443-476
    const int total = o.max_iterations;
    bool auto_scaling = params->robust_auto_scale && total > 0 && !facts->robust_is_none;
    if (auto_scaling && (params->robust_min_scale <= 0.0f || params->robust_min_scale >= params->robust_init_scale)) {
        std::fprintf(stderr, "[LIORegistration] Invalid geometry robust scale range; disabling auto scaling.\n");
        auto_scaling = false;
    }
    if (auto_scaling && (params->rotation_robust_min_scale <= 0.0f ||
                         params->rotation_robust_min_scale >= params->rotation_robust_init_scale)) {
        std::fprintf(stderr, "[LIORegistration] Invalid rotation robust scale range; disabling auto scaling.\n");
        auto_scaling = false;
    }
    if (auto_scaling && params->robust_auto_scaling_iter == 0) {
        std::fprintf(stderr, "[LIORegistration] auto_scaling_iter must be positive; disabling auto scaling.\n");
        auto_scaling = false;
    }
    s->levels = auto_scaling ? (params->robust_auto_scaling_iter < total ? params->robust_auto_scaling_iter : total) : 1;
    s->base_iterations = total / s->levels;
    s->extra_iterations = total % s->levels;
    s->robust_scale = auto_scaling ? params->robust_init_scale : facts->robust_default_scale;
    s->rotation_robust_scale = auto_scaling ? params->rotation_robust_init_scale : facts->rotation_robust_default_scale;
    s->robust_factor =
        s->levels > 1 ? powf(params->robust_min_scale / params->robust_init_scale, 1.0f / (float)(s->levels - 1)) : 1.0f;
    s->rotation_robust_factor = s->levels > 1 ? powf(params->rotation_robust_min_scale / params->rotation_robust_init_scale,
                                                     1.0f / (float)(s->levels - 1))
                                              : 1.0f;
    s->level = 0;
    sp::begin_level(*s);
    if (total == 0) s->done = 1;
    *out = s;
    return SP_OK;
}

extern "C" void sp_lio_stepper_destroy(sp_lio_stepper* s) { delete s; }

extern "C" int sp_lio_stepper_next(const sp_lio_stepper* s, sp_lio_request* out) {
    if (!s || !out) return SP_ERR_INVALID_ARGUMENT;
    out->want = s->done ? SP_OPT_WANT_DONE : s->phase == LIO_PHASE_LIN ? SP_OPT_WANT_LINEARIZE : SP_OPT_WANT_TRIAL;
    out->level = s->level;
    out->iteration = s->solver_iter;
    out->robust_scale = s->robust_scale;
    out->rotation_robust_scale = s->rotation_robust_scale;
    const sp::LioState& x = (!s->done && s->phase == LIO_PHASE_TRIAL_CANDIDATE) ? s->trial_state : s->op;
    sp::store_state(x, out->state);
    sp::state_to_pose(x, out->T);
    sp::state_to_pose(s->lin_state, out->T_lin);
    const int m = s->prm.opt.method;
    out->damping = m == SP_OPT_POWELL_DOGLEG ? s->radius : m == SP_OPT_LEVENBERG_MARQUARDT ? s->lm_lambda : s->prm.opt.gn_lambda;
    out->icp_weight = s->icp_weight;
    return SP_OK;
}

extern "C" int sp_lio_stepper_linearized(sp_lio_stepper* s, const sp_linearized* icp) {
    if (!s || !icp) return SP_ERR_INVALID_ARGUMENT;
    if (s->done || s->phase != LIO_PHASE_LIN) {
        sp_set_error("[sp_lio_stepper_linearized] no linearisation was asked for (sp_lio_stepper_next)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    using namespace sp;
    ++s->actual_iterations;
    s->lin_state = s->op;
    s->last_error = icp->error;
    s->last_inlier = icp->inlier;
    if (s->actual_iterations > 1 && s->imu_valid) {  // B:494-496
        float r[kN];
        manifold_residual(s->pred, s->op, r);
        matvec_n(s->H_imu, r, s->b_imu, kN);
    }
    s->icp_weight = 1.0f;  // B:498-502
    const float dof = (float)s->facts.residual_dim * (float)icp->inlier - 6.0f;
    if (dof > 0.0f && fabsf(icp->error) <= FLT_MAX && icp->error >= 0.0f)
        s->icp_weight = 1.0f / fmaxf(1.0f, 2.0f * icp->error / dof);

    sp_lio_linearized& lio = s->lio;
    std::memset(&lio, 0, sizeof(lio));
    add_icp_factor(&lio, icp, s->op.R, s->icp_weight);
    directional_weighting(&lio, s->prm.directional);
    if (s->imu_valid) {  // add_imu_factor (B:129-134)
        for (int i = 0; i < kN * kN; ++i) lio.H[i] += s->H_imu[i];
        for (int i = 0; i < kN; ++i) lio.b[i] += s->b_imu[i];
    } else {  // B:511-519
        const float reg = s->prm.invalid_regularization_factor;
        for (int i = kVel; i < kN; ++i) at(lio.H, i, i) += reg;
    }

    if (s->prm.opt.method == SP_OPT_GAUSS_NEWTON) {  // B:534-540
        float delta[kN];
        if (solve_damped(*s, s->prm.opt.gn_lambda, delta)) {
            bias_freeze(*s, delta);
            end_iteration(*s, true, false, delta);
        } else {
            end_iteration(*s, false, true, nullptr);
        }
        return SP_OK;
    }
    if (s->prm.opt.method == SP_OPT_POWELL_DOGLEG) s->radius = clamp_radius(*s, s->radius);  // B:587
    s->phase = LIO_PHASE_TRIAL_CURRENT;  // the current cost at the operating state (B:551, 586)
    return SP_OK;
}

extern "C" int sp_lio_stepper_trial(sp_lio_stepper* s, float error, uint32_t inlier) {
    if (!s) return SP_ERR_INVALID_ARGUMENT;
    if (s->done || s->phase == LIO_PHASE_LIN) {
        sp_set_error("[sp_lio_stepper_trial] no trial was asked for (sp_lio_stepper_next)");
        return SP_ERR_INVALID_ARGUMENT;
    }
    using namespace sp;
    (void)inlier;
    const sp_opt_params& o = s->prm.opt;
    if (s->phase == LIO_PHASE_TRIAL_CURRENT) {
        s->current_cost = s->icp_weight * error + imu_cost(*s, s->op);
        if (o.method == SP_OPT_LEVENBERG_MARQUARDT) {
            s->inner = 0;
            lm_next_trial(*s);
            return SP_OK;
        }
        const DoglegStepN dl = dogleg_step_n(s->lio.H, s->lio.b, s->radius, kN);  // B:588-597
        std::memcpy(s->trial_delta, dl.p, sizeof(s->trial_delta));
        s->dogleg_step_norm = dl.step_norm;
        bias_freeze(*s, s->trial_delta);
        float Hd[kN];
        matvec_n(s->lio.H, s->trial_delta, Hd, kN);
        s->predicted_reduction = -(dot_n(s->lio.b, s->trial_delta, kN) + 0.5f * dot_n(s->trial_delta, Hd, kN));
        if (s->predicted_reduction <= 0.0f) {
            s->radius = clamp_radius(*s, s->radius * o.dl_gamma_decrease);
            end_iteration(*s, false, false, nullptr);
            return SP_OK;
        }
        s->trial_state = retract(s->op, s->trial_delta);
        s->phase = LIO_PHASE_TRIAL_CANDIDATE;
        return SP_OK;
    }
    const float trial_cost = s->icp_weight * error + imu_cost(*s, s->trial_state);
    if (o.method == SP_OPT_LEVENBERG_MARQUARDT) {  // B:571-580
        if (trial_cost <= s->current_cost) {
            s->lm_lambda = clamp_lambda(*s, s->lm_lambda / o.lm_lambda_factor);
            end_iteration(*s, true, false, s->trial_delta);
        } else {
            s->lm_lambda = clamp_lambda(*s, s->lm_lambda * o.lm_lambda_factor);
            ++s->inner;
            lm_next_trial(*s);
        }
        return SP_OK;
    }
    const float rho = (s->current_cost - trial_cost) / s->predicted_reduction;  // B:602-620
    if (rho < o.dl_eta1) {
        s->radius = clamp_radius(*s, s->radius * o.dl_gamma_decrease);
        end_iteration(*s, false, false, nullptr);
        return SP_OK;
    }
    const float radius = s->radius;
    if (rho > o.dl_eta2 && s->dogleg_step_norm >= radius * 0.99f) s->radius = clamp_radius(*s, radius * o.dl_gamma_increase);
    end_iteration(*s, true, false, s->trial_delta);
    return SP_OK;
}

extern "C" int sp_lio_stepper_result(const sp_lio_stepper* s, sp_lio_result* out) {
    if (!s || !out) return SP_ERR_INVALID_ARGUMENT;
    using namespace sp;
    store_state(s->op, out->state);
    out->iterations = s->actual_iterations;
    out->inlier = s->last_inlier;
    out->error = s->last_error;
    out->converged = 1;
    // posterior_covariance (B:663-685)
    std::memcpy(out->posterior_covariance, s->P_prev, sizeof(s->P_prev));
    if (!s->has_H_undamped) return SP_OK;
    LdltN ldlt;
    ldlt.compute(s->H_undamped, kN);
    if (ldlt.positive()) { ldlt.inverse(out->posterior_covariance); return SP_OK; }
    float damped[225];
    std::memcpy(damped, s->H_undamped, sizeof(damped));
    for (int i = 0; i < kN; ++i) damped[i * kN + i] += 1e-4f;
    ldlt.compute(damped, kN);
    if (ldlt.positive()) { ldlt.inverse(out->posterior_covariance); return SP_OK; }
    std::fprintf(stderr, "[LIORegistration] WARNING: posterior covariance solve failed; keeping previous covariance.\n");
    return SP_OK;
}
