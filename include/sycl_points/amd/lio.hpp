// sycl_points facade for MI355X — tightly coupled LiDAR-inertial alignment.
//   algorithms/imu/imu_factor.hpp                 : imu::State, compute_manifold_residual, compute_imu_hessian_gradient,
//                                                   compute_imu_gradient
//   algorithms/lio/lio_linearized_result.hpp      : lio::LIOLinearizedResult
//   algorithms/lio/lio_registration_params.hpp    : lio::LIORobustScheduleParams, DirectionalIcpWeightingParams,
//                                                   LIORegistrationParams
//   algorithms/lio/lio_registration_result.hpp    : lio::LIORegistrationResult
//   algorithms/lio/lio_registration.hpp           : add_icp_factor, add_imu_factor, apply_directional_icp_weighting, solve_ldlt,
//                                                   retract, imu_to_lidar_jacobian, transform_covariance_*, LIORegistration
//   algorithms/registration/dogleg_step.hpp       : registration::DoglegStep<N>, compute_dogleg_step<N> (N = 6, 15)
// The 15x15 algebra and the optimiser's control flow are the C library's host code (sp_imu_*_host, sp_lio_*_host,
// sp_lio_stepper_*): one copy, shared with the Python mirror. LIORegistration::align serves the stepper's requests from its
// own Registration — compute_linearized_result and compute_error_frozen are the only device work; no kernel is LIO's own.
#pragma once
#include <cstring>
#include <limits>
#include <memory>
#include <tuple>

#include "registration.hpp"

namespace sycl_points {
namespace imu {

/// imu_factor.hpp:43-60 — the 15-DoF navigation state; error-state order [dp, dphi, dv, db_a, db_g]
struct State {
    static constexpr int kIdxPos = 0;
    static constexpr int kIdxRot = 3;
    static constexpr int kIdxVel = 6;
    static constexpr int kIdxAccBias = 9;
    static constexpr int kIdxGyrBias = 12;
    static constexpr int kDOF = 15;

    Eigen::Vector3f position = Eigen::Vector3f::Zero();
    Eigen::Matrix3f rotation = Eigen::Matrix3f::Identity();
    Eigen::Vector3f velocity = Eigen::Vector3f::Zero();
    Eigen::Vector3f accel_bias = Eigen::Vector3f::Zero();
    Eigen::Vector3f gyro_bias = Eigen::Vector3f::Zero();

    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
};

namespace detail {
/// the 21 floats of the C ABI: p3, R9 column-major, v3, b_a3, b_g3
struct PackedState {
    float v[21];
    explicit PackedState(const State& s) {
        for (int i = 0; i < 3; ++i) {
            v[i] = s.position(i);
            for (int j = 0; j < 3; ++j) v[3 + j * 3 + i] = s.rotation(i, j);
            v[12 + i] = s.velocity(i);
            v[15 + i] = s.accel_bias(i);
            v[18 + i] = s.gyro_bias(i);
        }
    }
};
inline State unpack_state(const float* v) {
    State s;
    for (int i = 0; i < 3; ++i) {
        s.position(i) = v[i];
        for (int j = 0; j < 3; ++j) s.rotation(i, j) = v[3 + j * 3 + i];
        s.velocity(i) = v[12 + i];
        s.accel_bias(i) = v[15 + i];
        s.gyro_bias(i) = v[18 + i];
    }
    return s;
}
}  // namespace detail

/// imu_factor.hpp:71-85
inline Eigen::Matrix<float, 15, 1> compute_manifold_residual(const State& x_pred, const State& x_op) {
    Eigen::Matrix<float, 15, 1> r;
    throw_on_error(sp_imu_manifold_residual_host(detail::PackedState(x_pred).v, detail::PackedState(x_op).v, r.data()));
    return r;
}
/// imu_factor.hpp:116-141
inline bool compute_imu_hessian_gradient(const State& x_pred, const State& x_op, const Eigen::Matrix<float, 15, 15>& P_pred,
                                         Eigen::Matrix<float, 15, 15>& H_imu, Eigen::Matrix<float, 15, 1>& b_imu) {
    int valid = 0;
    throw_on_error(sp_imu_hessian_gradient_host(detail::PackedState(x_pred).v, detail::PackedState(x_op).v, P_pred.data(),
                                                H_imu.data(), b_imu.data(), &valid));
    return valid != 0;
}
/// imu_factor.hpp:154-157
inline void compute_imu_gradient(const State& x_pred, const State& x_op, const Eigen::Matrix<float, 15, 15>& H_imu,
                                 Eigen::Matrix<float, 15, 1>& b_imu) {
    throw_on_error(sp_imu_gradient_host(detail::PackedState(x_pred).v, detail::PackedState(x_op).v, H_imu.data(), b_imu.data()));
}

}  // namespace imu

namespace algorithms {
namespace registration {

/// dogleg_step.hpp:13-18
template <int N>
struct DoglegStep {
    Eigen::Vector<float, N> p = Eigen::Vector<float, N>::Zero();
    float step_norm = 0.0f;
    float predicted_reduction = 0.0f;
};
/// dogleg_step.hpp:33-102, N = 6 or 15
template <int N>
inline DoglegStep<N> compute_dogleg_step(const Eigen::Matrix<float, N, N>& H, const Eigen::Vector<float, N>& g,
                                         float trust_region_radius) {
    static_assert(N == 6 || N == 15, "compute_dogleg_step: N must be 6 or 15");
    DoglegStep<N> result;
    throw_on_error(sp_dogleg_step_n_host(N, H.data(), g.data(), trust_region_radius, result.p.data(), &result.step_norm,
                                         &result.predicted_reduction));
    return result;
}

}  // namespace registration

namespace lio {

/// lio_linearized_result.hpp
struct LIOLinearizedResult {
    Eigen::Matrix<float, 15, 15> H = Eigen::Matrix<float, 15, 15>::Zero();
    Eigen::Matrix<float, 15, 1> b = Eigen::Matrix<float, 15, 1>::Zero();
    float error_icp = 0.0f;
    float error_imu = 0.0f;
    uint32_t inlier = 0;
};

/// lio_registration_params.hpp:11-18
struct LIORobustScheduleParams {
    bool auto_scale = false;
    float init_scale = 10.0f;
    float min_scale = 0.5f;
    float rotation_init_scale = 10.0f;
    float rotation_min_scale = 0.5f;
    size_t auto_scaling_iter = 4;
};
/// lio_registration_params.hpp:28-38
struct DirectionalIcpWeightingParams {
    bool enable = true;
    float trans_min_eigenvalue_per_inlier = 10.0f;
    float rot_min_eigenvalue_per_inlier = 10.0f;
    float trans_weak_direction_scale = 0.2f;
    float rot_weak_direction_scale = 0.2f;
};
/// lio_registration_params.hpp:41-49
struct LIORegistrationParams {
    size_t total_iterations = 10;
    registration::RegistrationConvergenceCriteria criteria;
    registration::RegistrationOptimizationParams optimization;
    LIORobustScheduleParams robust;
    float invalid_regularization_factor = 1e4f;
    DirectionalIcpWeightingParams directional_icp_weighting;
};
/// lio_registration_result.hpp
struct LIORegistrationResult {
    imu::State state;
    Eigen::Matrix<float, 15, 15> posterior_covariance = Eigen::Matrix<float, 15, 15>::Zero();
    registration::RegistrationResult registration_result;
};

namespace detail {
inline sp_lio_linearized to_c(const LIOLinearizedResult& r) {
    sp_lio_linearized c;
    std::memcpy(c.H, r.H.data(), sizeof(c.H));
    std::memcpy(c.b, r.b.data(), sizeof(c.b));
    c.error_icp = r.error_icp;
    c.error_imu = r.error_imu;
    c.inlier = r.inlier;
    c.pad = 0;
    return c;
}
inline void from_c(const sp_lio_linearized& c, LIOLinearizedResult& r) {
    std::memcpy(r.H.data(), c.H, sizeof(c.H));
    std::memcpy(r.b.data(), c.b, sizeof(c.b));
    r.error_icp = c.error_icp;
    r.error_imu = c.error_imu;
    r.inlier = c.inlier;
}
inline sp_linearized to_c(const registration::LinearizedResult& icp) {
    sp_linearized c;
    std::memset(&c, 0, sizeof(c));
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) c.H[i * 6 + j] = icp.H(i, j);
        c.b[i] = icp.b(i);
    }
    c.error = icp.error;
    c.inlier = icp.inlier;
    return c;
}
inline sp_lio_directional_params to_c(const DirectionalIcpWeightingParams& p) {
    return sp_lio_directional_params{p.enable ? 1 : 0, p.trans_min_eigenvalue_per_inlier, p.rot_min_eigenvalue_per_inlier,
                                     p.trans_weak_direction_scale, p.rot_weak_direction_scale};
}
inline sp_lio_params to_c(const LIORegistrationParams& p) {
    sp_lio_params c;
    const auto& o = p.optimization;
    c.opt = sp_opt_params{static_cast<int>(o.optimization_method), static_cast<int>(p.total_iterations), p.criteria.rotation,
                          p.criteria.translation, o.gn.lambda, static_cast<int>(o.lm.max_inner_iterations), o.lm.lambda_factor,
                          o.lm.init_lambda, o.lm.max_lambda, o.lm.min_lambda, o.dogleg.initial_trust_region_radius,
                          o.dogleg.min_trust_region_radius, o.dogleg.max_trust_region_radius, o.dogleg.eta1, o.dogleg.eta2,
                          o.dogleg.gamma_decrease, o.dogleg.gamma_increase};
    c.robust_auto_scale = p.robust.auto_scale ? 1 : 0;
    c.robust_init_scale = p.robust.init_scale;
    c.robust_min_scale = p.robust.min_scale;
    c.rotation_robust_init_scale = p.robust.rotation_init_scale;
    c.rotation_robust_min_scale = p.robust.rotation_min_scale;
    c.robust_auto_scaling_iter = static_cast<int>(p.robust.auto_scaling_iter);
    c.invalid_regularization_factor = p.invalid_regularization_factor;
    c.directional = to_c(p.directional_icp_weighting);
    return c;
}
}  // namespace detail

/// lio_registration.hpp:94-113
inline void add_icp_factor(LIOLinearizedResult& result, const registration::LinearizedResult& icp,
                           const Eigen::Matrix3f& R_world_lidar, float weight = 1.0f) {
    sp_lio_linearized c = detail::to_c(result);
    const sp_linearized lin = detail::to_c(icp);
    throw_on_error(sp_lio_add_icp_factor_host(&c, &lin, R_world_lidar.data(), weight));
    detail::from_c(c, result);
}
/// lio_registration.hpp:129-134
inline void add_imu_factor(LIOLinearizedResult& result, const Eigen::Matrix<float, 15, 15>& H_imu,
                           const Eigen::Matrix<float, 15, 1>& b_imu, float error = 0.0f) {
    for (int i = 0; i < 225; ++i) result.H.data()[i] += H_imu.data()[i];
    for (int i = 0; i < 15; ++i) result.b.data()[i] += b_imu.data()[i];
    result.error_imu = error;
}
/// lio_registration.hpp:144-202
inline void apply_directional_icp_weighting(LIOLinearizedResult& icp_factor, const DirectionalIcpWeightingParams& params) {
    sp_lio_linearized c = detail::to_c(icp_factor);
    const sp_lio_directional_params p = detail::to_c(params);
    throw_on_error(sp_lio_directional_weighting_host(&c, &p));
    detail::from_c(c, icp_factor);
}
/// lio_registration.hpp:224-238
inline bool solve_ldlt(const Eigen::Matrix<float, 15, 15>& H, const Eigen::Matrix<float, 15, 1>& b,
                       Eigen::Matrix<float, 15, 1>& delta, Eigen::Matrix<float, 15, 15>* P_post = nullptr) {
    int ok = 0;
    throw_on_error(sp_lio_solve_ldlt_host(H.data(), b.data(), delta.data(), P_post ? P_post->data() : nullptr, &ok));
    return ok != 0;
}
/// lio_registration.hpp:260-273
inline imu::State retract(const imu::State& state, const Eigen::Matrix<float, 15, 1>& delta) {
    float out[21];
    throw_on_error(sp_lio_retract_host(imu::detail::PackedState(state).v, delta.data(), out));
    return imu::detail::unpack_state(out);
}
/// lio_registration.hpp:308-323
inline Eigen::Matrix<float, 15, 15> imu_to_lidar_jacobian(const Eigen::Isometry3f& T_imu_to_lidar,
                                                          const Eigen::Matrix3f& R_world_lidar) {
    Eigen::Matrix<float, 15, 15> J;
    const TransformMatrix T = T_imu_to_lidar.matrix();
    throw_on_error(sp_lio_imu_to_lidar_jacobian_host(T.data(), R_world_lidar.data(), J.data()));
    return J;
}
/// lio_registration.hpp:340-345
inline Eigen::Matrix<float, 15, 15> transform_covariance_imu_to_lidar(const Eigen::Matrix<float, 15, 15>& P_imu,
                                                                      const Eigen::Isometry3f& T_imu_to_lidar,
                                                                      const Eigen::Matrix3f& R_world_lidar) {
    Eigen::Matrix<float, 15, 15> out;
    const TransformMatrix T = T_imu_to_lidar.matrix();
    throw_on_error(sp_lio_transform_covariance_host(P_imu.data(), T.data(), R_world_lidar.data(), 0, out.data()));
    return out;
}
/// lio_registration.hpp:366-381
inline Eigen::Matrix<float, 15, 15> transform_covariance_lidar_to_imu(const Eigen::Matrix<float, 15, 15>& P_lidar,
                                                                      const Eigen::Isometry3f& T_imu_to_lidar,
                                                                      const Eigen::Matrix3f& R_world_lidar) {
    Eigen::Matrix<float, 15, 15> out;
    const TransformMatrix T = T_imu_to_lidar.matrix();
    throw_on_error(sp_lio_transform_covariance_host(P_lidar.data(), T.data(), R_world_lidar.data(), 1, out.data()));
    return out;
}

/// lio_registration.hpp:384-690
class LIORegistration {
public:
    using Ptr = std::shared_ptr<LIORegistration>;

    LIORegistration(const sycl_utils::DeviceQueue& queue, const registration::RegistrationFactorParams& factor_params,
                    const LIORegistrationParams& params)
        : registration_(std::make_shared<registration::Registration>(queue, registration::RegistrationParams(factor_params))),
          factor_params_(factor_params),
          params_(params) {}

    const registration::Registration::Ptr& registration_backend() const { return registration_; }

    /// lio_registration.hpp:396-648: the stepper decides, the Registration linearises and evaluates
    LIORegistrationResult align(const PointCloudShared& source, const PointCloudShared& target, const knn::KNNBase& target_knn,
                                const imu::State& predicted_state, const Eigen::Matrix<float, 15, 15>& predicted_covariance,
                                const Eigen::Matrix<float, 15, 15>& previous_posterior_covariance, bool update_bias, float dt,
                                const TransformMatrix& previous_pose) {
        const sp_lio_params prm = detail::to_c(params_);
        const bool plane = factor_params_.reg_type == registration::RegType::POINT_TO_PLANE ||
                           factor_params_.reg_type == registration::RegType::GENZ;
        const sp_lio_factor_facts facts{plane ? 1 : 3, factor_params_.robust.type == robust::RobustLossType::NONE ? 1 : 0,
                                        factor_params_.robust.default_scale, factor_params_.rotation_constraint.robust.default_scale};
        registration::Registration::ExecutionOptions options;
        options.dt = dt;
        options.prev_pose = previous_pose;
        TransformMatrix initial_pose = TransformMatrix::Identity();
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) initial_pose(i, j) = predicted_state.rotation(i, j);
            initial_pose(i, 3) = predicted_state.position(i);
        }

        sp_lio_stepper* stepper = nullptr;
        throw_on_error(sp_lio_stepper_create(&prm, &facts, imu::detail::PackedState(predicted_state).v, predicted_covariance.data(),
                                             previous_posterior_covariance.data(), update_bias ? 1 : 0, &stepper));
        const std::unique_ptr<sp_lio_stepper, void (*)(sp_lio_stepper*)> guard(stepper, sp_lio_stepper_destroy);
        sp_lio_request req;
        for (;;) {
            throw_on_error(sp_lio_stepper_next(stepper, &req));
            if (req.want == SP_OPT_WANT_DONE) break;
            options.robust_scale = req.robust_scale;
            options.rotation_robust_scale = req.rotation_robust_scale;
            TransformMatrix pose;
            std::memcpy(pose.data(), req.T, sizeof(req.T));
            if (req.want == SP_OPT_WANT_LINEARIZE) {
                const sp_linearized lin =
                    detail::to_c(registration_->compute_linearized_result(source, target, target_knn, pose, initial_pose, options));
                throw_on_error(sp_lio_stepper_linearized(stepper, &lin));
            } else {
                const auto [error, inlier] = registration_->compute_error_frozen(source, target, pose, options);
                throw_on_error(sp_lio_stepper_trial(stepper, error, inlier));
            }
        }
        sp_lio_result res;
        throw_on_error(sp_lio_stepper_result(stepper, &res));

        LIORegistrationResult result;
        result.state = imu::detail::unpack_state(res.state);
        std::memcpy(result.posterior_covariance.data(), res.posterior_covariance, sizeof(res.posterior_covariance));
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) result.registration_result.T.matrix()(i, j) = result.state.rotation(i, j);
            result.registration_result.T.matrix()(i, 3) = result.state.position(i);
        }
        result.registration_result.converged = res.converged != 0;
        result.registration_result.iterations = res.iterations;
        result.registration_result.inlier = res.inlier;
        result.registration_result.error = res.error;
        return result;
    }

private:
    registration::Registration::Ptr registration_;
    registration::RegistrationFactorParams factor_params_;
    LIORegistrationParams params_;
};

}  // namespace lio
}  // namespace algorithms
}  // namespace sycl_points
