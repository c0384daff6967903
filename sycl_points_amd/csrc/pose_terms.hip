// Host-side pose-space terms of Registration::align that act on the reduced 6x6 system between the device reduction and
// the solve (registration.hpp:236-253): NL-Reg degenerate regularisation and the MAP prior, plus se3_log (sp_pose_math.h).
// Plain host arithmetic (the reference runs these on the host with Eigen); H is row-major as in sp_linearized.
#include <cmath>
#include <cstring>

#include "sp_common.h"
#include "sp_math.h"
#include "sp_pose_math.h"

void sp_set_error(const char* msg);

namespace sp {
namespace {

void add_weak_directions(const float* H, int o, float inlier, float threshold, float lambda, float* P) {
    if (!(threshold > 0.0f)) return;
    float blk[3][3], lam[3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) blk[i][j] = H[(o + i) * 6 + (o + j)];
    eigen_sym3(blk, lam, V);
    for (int e = 0; e < 3; ++e)
        if (lam[e] / inlier < threshold)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) P[(o + r) * 6 + (o + c)] += lambda * (V[r][e] * V[c][e]);
}

}  // namespace
}  // namespace sp

extern "C" void sp_se3_log_host(const float* T16, float* twist6) { sp::se3_log(sp::load_rigid_colmajor(T16), twist6); }

extern "C" int sp_degenerate_regularize_host(const sp_degenerate_reg_params* params, float* H36_rowmajor, float* b6,
                                             uint32_t inlier, const float* T_current16, const float* T_initial16) {
    if (!params || !H36_rowmajor || !b6 || !T_current16 || !T_initial16) return SP_ERR_INVALID_ARGUMENT;
    if (inlier == 0 || params->type == SP_DEGENERATE_REG_NONE) return SP_OK;
    if (params->type != SP_DEGENERATE_REG_NL_REG) {
        sp_set_error("[DegenerateRegularization] unknown type");
        return SP_ERR_INVALID_ARGUMENT;
    }
    const float n = (float)inlier, lambda = params->base_factor * n;
    float P[36] = {};
    sp::add_weak_directions(H36_rowmajor, 0, n, params->rot_eigenvalue_threshold, lambda, P);
    sp::add_weak_directions(H36_rowmajor, 3, n, params->trans_eigenvalue_threshold, lambda, P);
    float twist[6];
    sp::se3_log(sp::rigid_mul(sp::rigid_inverse(sp::load_rigid_colmajor(T_initial16)), sp::load_rigid_colmajor(T_current16)),
                twist);
    for (int i = 0; i < 6; ++i) {
        float s = 0.0f;
        for (int k = 0; k < 6; ++k) s += P[i * 6 + k] * twist[k];
        b6[i] += s;
        for (int j = 0; j < 6; ++j) H36_rowmajor[i * 6 + j] += P[i * 6 + j];
    }
    return SP_OK;
}

extern "C" int sp_map_prior_update_host(const sp_map_prior_params* params, const float* H_raw36_rowmajor, float error_raw,
                                        uint32_t inlier, const float* T_prev16, const float* T_pred16,
                                        sp_map_prior_state* state) {
    if (!params || !H_raw36_rowmajor || !T_prev16 || !T_pred16 || !state) return SP_ERR_INVALID_ARGUMENT;
    state->has_prior = 0;
    if (!params->enabled) return SP_OK;
    const float dof = 3.0f * (float)inlier - 6.0f;
    if (dof <= 0.0f) return SP_OK;
    if (!(fabsf(error_raw) <= FLT_MAX) || error_raw < 0.0f) return SP_OK;
    const float s_sq = fmaxf(1.0f, 2.0f * error_raw / dof);
    const sp::Rigid prev = sp::load_rigid_colmajor(T_prev16), pred = sp::load_rigid_colmajor(T_pred16);
    float Rrel[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 3; ++k) s += prev.R[k][i] * pred.R[k][j];
            Rrel[i][j] = s;
        }
    // predicted inter-frame motion in the body frame: AngleAxisf(R_rel) via its quaternion, and R_pred^T (t_pred - t_prev)
    float q[4], drot[3] = {0.0f, 0.0f, 0.0f}, dtr[3];
    sp::rot_to_quat(Rrel, q);
    float vn = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    if (q[3] < 0.0f) vn = -vn;
    if (vn != 0.0f) {
        const float angle = 2.0f * atan2f(vn, fabsf(q[3]));
        for (int i = 0; i < 3; ++i) drot[i] = (q[i] / vn) * angle;
    }
    for (int i = 0; i < 3; ++i) {
        float s = 0.0f;
        for (int k = 0; k < 3; ++k) s += pred.R[k][i] * (pred.t[k] - prev.t[k]);
        dtr[i] = s;
    }
    float Rd[6];  // R = Q^-1, diagonal
    for (int i = 0; i < 3; ++i) {
        Rd[i] = 1.0f / (fabsf(drot[i]) * (params->rot_vel_sigma * params->rot_vel_sigma) +
                        params->rot_base_sigma * params->rot_base_sigma);
        Rd[3 + i] = 1.0f / (fabsf(dtr[i]) * (params->trans_vel_sigma * params->trans_vel_sigma) +
                            params->trans_base_sigma * params->trans_base_sigma);
    }
    // H_curr = Ad^T (H_raw / s^2) Ad, Ad = diag(R_rel, R_rel): block by block
    float Hc[36], tmp[36];
    auto Ad = [&](int r, int c) { return ((r < 3) == (c < 3)) ? Rrel[r % 3][c % 3] : 0.0f; };
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 6; ++k) s += Ad(k, i) * (H_raw36_rowmajor[k * 6 + j] / s_sq);
            tmp[i * 6 + j] = s;
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            float s = 0.0f;
            for (int k = 0; k < 6; ++k) s += tmp[i * 6 + k] * Ad(k, j);
            Hc[i * 6 + j] = s;
        }
    for (int i = 0; i < 6; ++i) Hc[i * 6 + i] += Rd[i];
    // Omega = R - R (H + R)^-1 R (matrix inversion lemma; H + R is positive definite)
    sp::LdltScratch w;
    for (int c = 0; c < 6; ++c) {
        float rhs[6] = {}, x[6];
        rhs[c] = Rd[c];
        if (!sp::ldlt6_solve(Hc, rhs, x, w)) return SP_OK;  // no prior this frame (map_prior.hpp:166)
        for (int r = 0; r < 6; ++r) state->omega[r * 6 + c] = (r == c ? Rd[c] : 0.0f) - Rd[r] * x[r];
    }
    sp::store_rigid_colmajor(sp::rigid_inverse(pred), state->T_pred_inv);
    state->has_prior = 1;
    return SP_OK;
}

extern "C" float sp_map_prior_apply_host(const sp_map_prior_state* state, const float* T_est16, float* H36_rowmajor,
                                         float* b6, float* error) {
    if (!state || !state->has_prior || !T_est16) return 0.0f;
    float e[6], Oe[6];
    sp::se3_log(sp::rigid_mul(sp::load_rigid_colmajor(state->T_pred_inv), sp::load_rigid_colmajor(T_est16)), e);
    float cost = 0.0f;
    for (int i = 0; i < 6; ++i) {
        float s = 0.0f;
        for (int k = 0; k < 6; ++k) s += state->omega[i * 6 + k] * e[k];
        Oe[i] = s;
    }
    for (int i = 0; i < 6; ++i) cost += e[i] * Oe[i];
    cost *= 0.5f;
    if (H36_rowmajor && b6) {
        for (int i = 0; i < 6; ++i) {
            b6[i] += Oe[i];
            for (int j = 0; j < 6; ++j) H36_rowmajor[i * 6 + j] += state->omega[i * 6 + j];
        }
        if (error) *error += cost;
    }
    return cost;
}
