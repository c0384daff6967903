// sycl_points facade for MI355X — the per-frame odometry loop.
//   utils/time_utils.hpp                          : time_utils::measure_execution
//   algorithms/imu/imu_initial_alignment.hpp      : imu::InitialAlignmentParams, InitialAlignmentResult, estimate_initial_alignment,
//                                                   detail::yaw_from_rotation, InitialAlignmentEstimator
//   algorithms/imu/imu_velocity_corrector.hpp     : imu::IMUVelocityCorrector
//   pipeline/adaptive_motion_predictor.hpp        : pipeline::lidar_odometry::AdaptiveMotionPredictor
//   pipeline/motion_predictor.hpp                 : MotionPredictionMode (+ strings), MotionPredictionCandidates, MotionPredictor
//   pipeline/odometry_common_params.hpp           : pipeline::odometry::SubmapMapType (+ strings), CommonParameters
//   pipeline/lidar_odometry_params.hpp            : pipeline::lidar_odometry::Parameters
//   pipeline/pointcloud_processing.hpp            : pipeline::pointcloud_processing::ProcessingContext, PCProcessor
//   pipeline/submapping.hpp                       : pipeline::submapping::Submap
//   pipeline/lidar_odometry.hpp                   : pipeline::lidar_odometry::LiDAROdometryPipeline
//   pipeline/lidar_inertial_odometry_params.hpp   : pipeline::lidar_inertial_odometry::Parameters
//   pipeline/lidar_inertial_odometry.hpp          : pipeline::lidar_inertial_odometry::LidarInertialOdometryPipeline
//   (what the two loops hold word for word lives once, in pipeline::odometry::PipelineCommon)
// Callers only: every per-point stage is a class of the other amd/*.hpp files, i.e. a kernel of the C library; the 3x3 / 4x4 /
// 15x15 arithmetic between them is the library's host code (csrc/odometry_host.hip, csrc/lio_host.hip), shared with the Python
// wrappers. No kernel is launched from this file directly and no point data crosses to the host in it.
#pragma once
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <deque>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <numbers>
#include <optional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "imu.hpp"
#include "lio.hpp"
#include "mapping.hpp"
#include "registration.hpp"

namespace sycl_points {

// ------------------------------------------------------------------------------------------------ utils/time_utils.hpp
namespace time_utils {

/// time_utils.hpp:37-55 — runs func(args...), ADDS the elapsed microseconds (steady clock) to elapsed_time, returns func's result
template <typename TimeType = double, typename Func, typename... Args>
auto measure_execution(Func&& func, TimeType& elapsed_time, Args&&... args) -> decltype(func(std::forward<Args>(args)...)) {
    const auto start = std::chrono::steady_clock::now();
    if constexpr (std::is_void_v<decltype(func(std::forward<Args>(args)...))>) {
        func(std::forward<Args>(args)...);
        elapsed_time += std::chrono::duration<TimeType, std::micro>(std::chrono::steady_clock::now() - start).count();
        return;
    } else {
        auto result = func(std::forward<Args>(args)...);
        elapsed_time += std::chrono::duration<TimeType, std::micro>(std::chrono::steady_clock::now() - start).count();
        return result;
    }
}

}  // namespace time_utils

namespace detail {
// the rotation of an isometry read and written entry by entry (the no-Eigen subset has no writable linear())
inline Eigen::Matrix3f rotation_of(const Eigen::Isometry3f& T) {
    Eigen::Matrix3f R;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R(i, j) = T.matrix()(i, j);
    return R;
}
inline void set_rotation(Eigen::Isometry3f& T, const Eigen::Matrix3f& R) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T.matrix()(i, j) = R(i, j);
}
inline Eigen::Isometry3f isometry_of(const TransformMatrix& M) {
    Eigen::Isometry3f T = Eigen::Isometry3f::Identity();
    T.matrix() = M;
    return T;
}
inline std::string upper(const std::string& str) {
    std::string u = str;
    std::transform(u.begin(), u.end(), u.begin(), [](unsigned char c) { return std::toupper(c); });
    return u;
}
}  // namespace detail

// ------------------------------------------------------------------------------------------------ IMU initial alignment
namespace imu {

/// imu_initial_alignment.hpp:18-46
struct InitialAlignmentParams {
    bool enable = true;
    float required_duration_sec = 1.0f;
    float max_gyro_std = 0.01f;
    float max_accel_std = 0.2f;
    float max_accel_norm_error = 0.5f;
    bool estimate_gyro_bias = true;
    float max_wait_sec = 5.0f;
};

/// imu_initial_alignment.hpp:54-65
struct InitialAlignmentResult {
    bool success = false;
    Eigen::Matrix3f R_world_imu = Eigen::Matrix3f::Identity();
    Eigen::Vector3f gyro_bias = Eigen::Vector3f::Zero();
    Eigen::Vector3f accel_mean = Eigen::Vector3f::Zero();
    Eigen::Vector3f gyro_std = Eigen::Vector3f::Zero();
    Eigen::Vector3f accel_std = Eigen::Vector3f::Zero();
    float accel_norm = 0.0f;
    float roll_rad = 0.0f;
    float pitch_rad = 0.0f;
    std::string error_message;
};

/// imu_initial_alignment.hpp:85-204 — the C library's sp_initial_alignment_host on the buffer's samples
inline InitialAlignmentResult estimate_initial_alignment(const std::deque<IMUMeasurement>& imu_buffer,
                                                         const Eigen::Vector3f& gravity_world, const InitialAlignmentParams& params,
                                                         const IMUBias& current_bias, bool bypass_stationarity = false) {
    std::vector<double> stamps;
    std::vector<float> gyro_accel;
    stamps.reserve(imu_buffer.size());
    gyro_accel.reserve(6 * imu_buffer.size());
    for (const IMUMeasurement& m : imu_buffer) {
        stamps.push_back(m.timestamp);
        for (int k = 0; k < 3; ++k) gyro_accel.push_back(m.gyro[k]);
        for (int k = 0; k < 3; ++k) gyro_accel.push_back(m.accel[k]);
    }
    const sp_initial_alignment_params p{params.required_duration_sec, params.max_gyro_std, params.max_accel_std,
                                        params.max_accel_norm_error, params.estimate_gyro_bias ? 1 : 0};
    sp_initial_alignment_result r;
    throw_on_error(sp_initial_alignment_host(stamps.data(), gyro_accel.data(), stamps.size(), gravity_world.data(), &p,
                                             detail::Bias6(current_bias).v, bypass_stationarity ? 1 : 0, &r));
    InitialAlignmentResult res;
    res.success = r.success != 0;
    for (int k = 0; k < 9; ++k) res.R_world_imu.data()[k] = r.R_world_imu[k];
    for (int k = 0; k < 3; ++k) {
        res.gyro_bias[k] = r.gyro_bias[k];
        res.accel_mean[k] = r.accel_mean[k];
        res.gyro_std[k] = r.gyro_std[k];
        res.accel_std[k] = r.accel_std[k];
    }
    res.accel_norm = r.accel_norm;
    res.roll_rad = r.roll_rad;
    res.pitch_rad = r.pitch_rad;
    res.error_message = r.error_message;
    return res;
}

namespace detail {
/// imu_initial_alignment.hpp:211-218
inline float yaw_from_rotation(const Eigen::Matrix3f& R) { return sp_yaw_from_rotation_host(R.data()); }
}  // namespace detail

/// imu_initial_alignment.hpp:236-345 — the wait / timeout / forced-alignment logic around estimate_initial_alignment
class InitialAlignmentEstimator {
public:
    using Ptr = std::shared_ptr<InitialAlignmentEstimator>;

    enum class Status : std::int8_t {
        success = 0,
        waiting,  ///< not enough data / not stationary yet: keep polling
    };

    struct Output {
        Status status = Status::waiting;
        std::string error_message;  ///< set with Status::waiting
        Eigen::Matrix3f R_gravity_lidar = Eigen::Matrix3f::Identity();  ///< gravity-aligned LiDAR rotation, yaw ~ 0
        Eigen::Vector3f gyro_bias = Eigen::Vector3f::Zero();
        float roll_rad = 0.0f;
        float pitch_rad = 0.0f;
        float accel_norm = 0.0f;
    };

    InitialAlignmentEstimator(const InitialAlignmentParams& params, const Eigen::Vector3f& gravity_world,
                              const Eigen::Isometry3f& T_imu_to_lidar)
        : params_(params), gravity_world_(gravity_world), T_imu_to_lidar_(T_imu_to_lidar) {}

    bool enabled() const { return params_.enable; }
    bool is_done() const { return done_; }

    /// imu_initial_alignment.hpp:273-337
    Output try_align(double scan_timestamp, const std::deque<IMUMeasurement>& imu_buffer, const IMUBias& current_bias) {
        Output out;
        if (done_) {
            out.status = Status::success;
            return out;
        }
        if (alignment_start_timestamp_ < 0.0) alignment_start_timestamp_ = scan_timestamp;
        const double elapsed = scan_timestamp - alignment_start_timestamp_;
        const bool timeout_reached = params_.max_wait_sec > 0.0f && elapsed >= static_cast<double>(params_.max_wait_sec);

        auto result = estimate_initial_alignment(imu_buffer, gravity_world_, params_, current_bias, /*bypass_stationarity=*/false);
        if (!result.success && timeout_reached) {
            result = estimate_initial_alignment(imu_buffer, gravity_world_, params_, current_bias, /*bypass_stationarity=*/true);
            if (result.success)
                std::cerr << "[InitialAlignment] initial alignment FORCED after " << elapsed
                          << "s (robot was not detected stationary). gyro_bias may be biased; "
                          << "drift performance can degrade until convergence." << std::endl;
        }
        if (!result.success) {
            out.status = Status::waiting;
            out.error_message = result.error_message;
            const double span = imu_buffer.size() >= 2 ? (imu_buffer.back().timestamp - imu_buffer.front().timestamp) : 0.0;
            std::cerr << "[InitialAlignment] waiting initial alignment: " << result.error_message << " (samples=" << imu_buffer.size()
                      << ", buffer_span=" << span << "s, required=" << params_.required_duration_sec << "s, elapsed=" << elapsed
                      << "s/" << params_.max_wait_sec << "s, accel_mean_norm=" << result.accel_norm << ", gyro_std=["
                      << result.gyro_std[0] << " " << result.gyro_std[1] << " " << result.gyro_std[2] << "], accel_std=["
                      << result.accel_std[0] << " " << result.accel_std[1] << " " << result.accel_std[2] << "])" << std::endl;
            return out;
        }
        // R_gravity_lidar = R_world_imu_aligned * R_imu_to_lidar^T (:315-320)
        const Eigen::Matrix3f R_imu_to_lidar = sycl_points::detail::rotation_of(T_imu_to_lidar_);
        out.status = Status::success;
        out.R_gravity_lidar = result.R_world_imu * R_imu_to_lidar.transpose();
        out.gyro_bias = result.gyro_bias;
        out.roll_rad = result.roll_rad;
        out.pitch_rad = result.pitch_rad;
        out.accel_norm = result.accel_norm;
        done_ = true;
        std::cout << "[InitialAlignment] initial alignment done: roll=" << result.roll_rad * 180.0f / std::numbers::pi_v<float>
                  << " deg, pitch=" << result.pitch_rad * 180.0f / std::numbers::pi_v<float> << " deg, |a|=" << result.accel_norm
                  << " m/s^2, gyro_bias=[" << result.gyro_bias[0] << " " << result.gyro_bias[1] << " " << result.gyro_bias[2] << "]"
                  << std::endl;
        return out;
    }

private:
    InitialAlignmentParams params_;
    Eigen::Vector3f gravity_world_;
    Eigen::Isometry3f T_imu_to_lidar_;
    bool done_ = false;
    double alignment_start_timestamp_ = -1.0;
};

/// imu_velocity_corrector.hpp:30-83 — the ICP-corrected velocity at which the next IMU window starts
class IMUVelocityCorrector {
public:
    using Ptr = std::shared_ptr<IMUVelocityCorrector>;

    /// imu_velocity_corrector.hpp:42-54
    Eigen::Vector3f get_reset_velocity(const IMUPreintegration& preintegration, const IMUBias& bias,
                                       const Eigen::Vector3f& fallback_v_world) {
        const Eigen::Vector3f v_reset = corrected_v_valid_ ? corrected_v_world_ : fallback_v_world;
        corrected_v_valid_ = false;
        const PreintegrationResult snap = preintegration.get_corrected(bias);
        set_snapshot(snap.Delta_v, snap.Delta_p, static_cast<float>(snap.dt_total));
        return v_reset;
    }
    /// the snapshot get_reset_velocity takes from the integrator, given directly (MI355X extension: a test needs no integrator)
    void set_snapshot(const Eigen::Vector3f& delta_v, const Eigen::Vector3f& delta_p, float dt) {
        snapshot_delta_v_ = delta_v;
        snapshot_delta_p_ = delta_p;
        snapshot_dt_ = dt;
        snapshot_valid_ = true;
    }
    /// imu_velocity_corrector.hpp:62-71:
    ///   v_reset_corrected = (disp_icp - 0.5 g dt^2 - R dp) / dt;   v_k = v_reset_corrected + g dt + R dv
    void update(const Eigen::Vector3f& disp_icp, const Eigen::Matrix3f& R_world_imu, const Eigen::Vector3f& gravity) {
        if (!snapshot_valid_ || snapshot_dt_ <= 0.0f) return;
        const float dt = snapshot_dt_;
        const Eigen::Vector3f v_reset_corrected = (disp_icp - gravity * 0.5f * dt * dt - R_world_imu * snapshot_delta_p_) / dt;
        corrected_v_world_ = v_reset_corrected + gravity * dt + R_world_imu * snapshot_delta_v_;
        corrected_v_valid_ = true;
        snapshot_valid_ = false;
    }

private:
    Eigen::Vector3f snapshot_delta_v_ = Eigen::Vector3f::Zero();
    Eigen::Vector3f snapshot_delta_p_ = Eigen::Vector3f::Zero();
    float snapshot_dt_ = 0.0f;
    bool snapshot_valid_ = false;
    Eigen::Vector3f corrected_v_world_ = Eigen::Vector3f::Zero();
    bool corrected_v_valid_ = false;
};

}  // namespace imu

namespace pipeline {

// ------------------------------------------------------------------------------------------------ motion prediction
namespace lidar_odometry {

/// pipeline/motion_predictor.hpp:17-42
enum class MotionPredictionMode {
    LIDAR_CV = SP_MOTION_LIDAR_CV,
    GYRO_LIDAR_CV = SP_MOTION_GYRO_LIDAR_CV,
    IMU_SE3 = SP_MOTION_IMU_SE3,
};
inline MotionPredictionMode MotionPredictionMode_from_string(const std::string& str) {
    const std::string u = sycl_points::detail::upper(str);
    if (u == "LIDAR_CV") return MotionPredictionMode::LIDAR_CV;
    if (u == "GYRO_LIDAR_CV") return MotionPredictionMode::GYRO_LIDAR_CV;
    if (u == "IMU_SE3") return MotionPredictionMode::IMU_SE3;
    throw std::runtime_error("[MotionPredictionMode_from_string] Invalid motion prediction mode '" + str + "'");
}
inline std::string MotionPredictionMode_to_string(const MotionPredictionMode mode) {
    switch (mode) {
        case MotionPredictionMode::LIDAR_CV: return "LIDAR_CV";
        case MotionPredictionMode::GYRO_LIDAR_CV: return "GYRO_LIDAR_CV";
        case MotionPredictionMode::IMU_SE3: return "IMU_SE3";
    }
    throw std::runtime_error("[MotionPredictionMode_to_string] Invalid motion prediction mode");
}

/// pipeline/motion_predictor.hpp:44-47
struct MotionPredictionCandidates {
    std::optional<Eigen::Matrix3f> gyro_delta_rotation_lidar;
    std::optional<Eigen::Isometry3f> imu_se3_pose;
};

namespace detail {
/// both predictors over sp_motion_predict_host: `state` holds the velocity averages of the caller
struct MotionAxis { float factor_min, factor_max, min_eigenvalue_low, min_eigenvalue_high; };
inline Eigen::Isometry3f motion_predict(const MotionAxis& rotation, const MotionAxis& translation, float velocity_ema_alpha,
                                        MotionPredictionMode mode, sp_motion_predict_state& state,
                                        const Eigen::Vector3f& linear_velocity, const Eigen::AngleAxisf& angular_velocity,
                                        const Eigen::Isometry3f& odom, float dt,
                                        const algorithms::registration::RegistrationResult::Ptr& reg_result, bool registrated,
                                        const MotionPredictionCandidates& candidates, float* factors2) {
    const sp_motion_predict_params p{{rotation.factor_min, rotation.factor_max, rotation.min_eigenvalue_low, rotation.min_eigenvalue_high},
                                     {translation.factor_min, translation.factor_max, translation.min_eigenvalue_low,
                                      translation.min_eigenvalue_high},
                                     velocity_ema_alpha, int(mode)};
    const float angle = angular_velocity.angle();
    const Eigen::Vector3f axis = angular_velocity.axis();
    const float rotvec[3] = {axis[0] * angle, axis[1] * angle, axis[2] * angle};  // adaptive_motion_predictor.hpp:106
    const bool use_result = registrated && reg_result != nullptr;
    float H36[36];
    if (use_result)
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) H36[i * 6 + j] = reg_result->H_raw(i, j);
    const TransformMatrix odom_m = odom.matrix();
    Eigen::Matrix3f gyro;
    TransformMatrix se3;
    if (candidates.gyro_delta_rotation_lidar) gyro = *candidates.gyro_delta_rotation_lidar;
    if (candidates.imu_se3_pose) se3 = candidates.imu_se3_pose->matrix();
    TransformMatrix out;
    throw_on_error(sp_motion_predict_host(&p, &state, linear_velocity.data(), rotvec, odom_m.data(), dt, use_result ? H36 : nullptr,
                                          use_result ? reg_result->inlier : 0u, use_result ? 1 : 0,
                                          candidates.gyro_delta_rotation_lidar ? gyro.data() : nullptr,
                                          candidates.imu_se3_pose ? se3.data() : nullptr, out.data(), factors2));
    return sycl_points::detail::isometry_of(out);
}
}  // namespace detail

/// pipeline/adaptive_motion_predictor.hpp:17-142 — constant-velocity prediction, damped where the last registration was well
/// constrained (the smallest eigenvalue of H_raw's rotation / translation block per inlier)
class AdaptiveMotionPredictor {
public:
    using Ptr = std::shared_ptr<AdaptiveMotionPredictor>;

    struct Params {
        struct AdaptiveAxis {
            float factor_min = 0.2f;
            float factor_max = 1.0f;
            float min_eigenvalue_low = 1.0f;
            float min_eigenvalue_high = 10.0f;
        };
        struct Adaptive {
            AdaptiveAxis rotation = {.factor_min = 0.2f, .factor_max = 1.0f, .min_eigenvalue_low = 5.0f, .min_eigenvalue_high = 10.0f};
            AdaptiveAxis translation;
        };
        bool verbose = false;
        float velocity_ema_alpha = 1.0f;  // 1.0 = the raw velocity, 0.0 = frozen
        Adaptive adaptive;
    };

    explicit AdaptiveMotionPredictor(const Params& params) : params_(params) {}

    /// adaptive_motion_predictor.hpp:54-133
    Eigen::Isometry3f predict(const Eigen::Vector3f& linear_velocity, const Eigen::AngleAxisf& angular_velocity,
                              const Eigen::Isometry3f& odom, float dt,
                              const algorithms::registration::RegistrationResult::Ptr& reg_result, bool registrated) {
        return predict_with(MotionPredictionMode::LIDAR_CV, linear_velocity, angular_velocity, odom, dt, reg_result, registrated, {});
    }
    /// MI355X extension: the (rotation, translation) factors of the latest predict
    std::pair<float, float> last_factors() const { return {factors_[0], factors_[1]}; }

private:
    friend class MotionPredictor;
    Eigen::Isometry3f predict_with(MotionPredictionMode mode, const Eigen::Vector3f& linear_velocity,
                                   const Eigen::AngleAxisf& angular_velocity, const Eigen::Isometry3f& odom, float dt,
                                   const algorithms::registration::RegistrationResult::Ptr& reg_result, bool registrated,
                                   const MotionPredictionCandidates& candidates) {
        const auto& r = params_.adaptive.rotation;
        const auto& t = params_.adaptive.translation;
        const Eigen::Isometry3f T = detail::motion_predict(
            {r.factor_min, r.factor_max, r.min_eigenvalue_low, r.min_eigenvalue_high},
            {t.factor_min, t.factor_max, t.min_eigenvalue_low, t.min_eigenvalue_high}, params_.velocity_ema_alpha, mode, state_,
            linear_velocity, angular_velocity, odom, dt, reg_result, registrated, candidates, factors_);
        if (params_.verbose)
            std::cout << "[motion predictor] rot: factor=" << factors_[0] << ", trans: factor=" << factors_[1] << std::endl;
        return T;
    }
    Params params_;
    sp_motion_predict_state state_{};  // the velocity averages (:140-141)
    float factors_[2] = {1.0f, 1.0f};
};

/// pipeline/motion_predictor.hpp:50-83 — selects and combines the available initial-pose predictions
class MotionPredictor {
public:
    using Ptr = std::shared_ptr<MotionPredictor>;

    struct Params : AdaptiveMotionPredictor::Params {
        MotionPredictionMode mode = MotionPredictionMode::GYRO_LIDAR_CV;
    };

    explicit MotionPredictor(const Params& params) : params_(params), lidar_cv_predictor_(params) {}

    /// motion_predictor.hpp:60-76
    Eigen::Isometry3f predict(const Eigen::Vector3f& linear_velocity, const Eigen::AngleAxisf& angular_velocity,
                              const Eigen::Isometry3f& odom, float dt,
                              const algorithms::registration::RegistrationResult::Ptr& reg_result, bool registrated,
                              const MotionPredictionCandidates& candidates = {}) {
        return lidar_cv_predictor_.predict_with(params_.mode, linear_velocity, angular_velocity, odom, dt, reg_result, registrated,
                                                candidates);
    }

private:
    Params params_;
    AdaptiveMotionPredictor lidar_cv_predictor_;
};

}  // namespace lidar_odometry

// ------------------------------------------------------------------------------------------------ parameters
namespace odometry {

/// pipeline/odometry_common_params.hpp:19-44
enum class SubmapMapType {
    OCCUPANCY_GRID_MAP = 0,
    VOXEL_HASH_MAP,
};
inline SubmapMapType SubmapMapType_from_string(const std::string& str) {
    const std::string u = sycl_points::detail::upper(str);
    if (u == "OCCUPANCY_GRID_MAP") return SubmapMapType::OCCUPANCY_GRID_MAP;
    if (u == "VOXEL_HASH_MAP") return SubmapMapType::VOXEL_HASH_MAP;
    throw std::runtime_error("[SubmapMapType_from_string] Invalid submap map type '" + str + "'");
}
inline std::string SubmapMapType_to_string(const SubmapMapType type) {
    switch (type) {
        case SubmapMapType::OCCUPANCY_GRID_MAP: return "OCCUPANCY_GRID_MAP";
        case SubmapMapType::VOXEL_HASH_MAP: return "VOXEL_HASH_MAP";
    }
    throw std::runtime_error("[SubmapMapType_to_string] Invalid submap map type");
}

/// pipeline/odometry_common_params.hpp:47-227 — every field and default of the reference
struct CommonParameters {
    struct Device {  // kept for source compatibility and ignored: the queue is the facade's DeviceQueue on device 0
        std::string vendor = "intel";
        std::string type = "gpu";
    };
    struct Scan {
        struct IntensityCorrection {
            bool enable = true;
            float exp = 2.0f;
            float scale = 1e-3f;
            float min_intensity = 0.0f;
            float max_intensity = 1.0f;
            float ref_distance = 1.0f;
            float angle_exponent = 0.0f;
        };
        struct Downsampling {
            struct Voxel {
                bool enable = false;
                float size = 1.0f;
            };
            struct Polar {
                bool enable = true;
                float distance_size = 1.0f;
                float elevation_size = 3.0f * std::numbers::pi_v<float> / 180.0f;
                float azimuth_size = 3.0f * std::numbers::pi_v<float> / 180.0f;
                std::string coord_system = "CAMERA";
            };
            struct Random {
                bool enable = true;
                size_t num = 5000;
            };
            Voxel voxel;
            Polar polar;
            Random random;
        };
        struct Preprocess {
            struct BoxFilter {
                bool enable = true;
                float min = 2.0f;
                float max = 50.0f;
            };
            struct AngleIncidenceFilter {
                bool enable = true;
                float min_angle = 0.0f;
                float max_angle = 80.0f * std::numbers::pi_v<float> / 180.0f;
            };
            BoxFilter box_filter;
            AngleIncidenceFilter angle_incidence_filter;
        };
        struct IntensityGaussian {
            bool enable = false;
            size_t neighbor_num = 10;
            float sigma_azimuth = 0.3f;
            float sigma_elevation = 0.5f;
            float sigma_range = 0.05f;
        };
        struct IntensityLocalMeanNorm {
            bool enable = false;
            size_t neighbor_num = 10;
            float sigma_azimuth = 0.3f;
            float sigma_elevation = 0.5f;
            float sigma_range = 0.05f;
            float mean_min = 1e-3f;
        };
        struct EnhancedReflectivity {  // consumed by the caller that owns the messages (ros2::EnhancedReflectivityCorrector); `enable` switches intensity_correction off
            bool enable = false;
            float clip_max = 5.0f;
            float ring_mean_ema_alpha = 0.5f;
        };
        IntensityCorrection intensity_correction;
        IntensityGaussian intensity_gaussian;
        IntensityLocalMeanNorm intensity_local_mean_norm;
        EnhancedReflectivity enhanced_reflectivity;
        Downsampling downsampling;
        Preprocess preprocess;
    };
    struct Submap {
        struct Keyframe {
            float inlier_ratio_threshold = 0.7f;
            float distance_threshold = 2.0f;
            float angle_threshold_degrees = 20.0f;
            float time_threshold_seconds = 1.0f;
        };
        struct OccupancyGridMap {
            float log_odds_hit = 0.8f;
            float log_odds_miss = -0.05f;
            float log_odds_limits_min = -1.0f;
            float log_odds_limits_max = 4.0f;
            float occupied_threshold = 0.5f;
            bool enable_free_space_updates = true;
            bool enable_pruning = true;
            size_t stale_frame_threshold = 100U;
        };
        SubmapMapType map_type = SubmapMapType::OCCUPANCY_GRID_MAP;
        float voxel_size = 1.0f;
        float max_distance_range = 30.0f;
        size_t point_random_sampling_num = 512;
        float weighted_sampling_ratio = 0.8f;
        Keyframe keyframe;
        OccupancyGridMap occupancy_grid_map;
    };
    struct CovarianceEstimation {
        struct MEstimation {
            bool enable = true;
            algorithms::robust::RobustLossType type = algorithms::robust::RobustLossType::GEMAN_MCCLURE;
            float mad_scale = 1.0f;
            float min_robust_scale = 5.0f;
            size_t max_iterations = 1;
        };
        size_t neighbor_num = 10;
        MEstimation m_estimation;
    };
    struct IMU {
        bool enable = false;
        Eigen::Isometry3f T_imu_to_lidar = Eigen::Isometry3f::Identity();  ///< p_lidar = T_imu_to_lidar * p_imu
        imu::IMUPreintegrationParams preintegration;
        imu::IMUBias bias;
        double buffer_duration_sec = 1.0;
        struct Deskew {
            bool enable = false;
            bool gyro_only = false;
        };
        Deskew deskew;
        imu::InitialAlignmentParams initial_alignment;
    };
    struct Registration {
        size_t min_num_points = 100;
        algorithms::registration::RegistrationFactorParams factor;
    };
    struct Pose {
        Eigen::Isometry3f initial = Eigen::Isometry3f::Identity();
    };

    Device device;
    Scan scan;
    Submap submap;
    CovarianceEstimation covariance_estimation;
    IMU imu;
    Registration registration;
    algorithms::registration::RegistrationRandomSamplingParams registration_sampling;
    Pose pose;
};

}  // namespace odometry

namespace lidar_odometry {

/// pipeline/lidar_odometry_params.hpp:12-51
struct Parameters : public odometry::CommonParameters {
    using MotionPrediction = MotionPredictor::Params;

    struct LO {
        struct Registration {
            using Criteria = algorithms::registration::RegistrationConvergenceCriteria;
            size_t max_iterations = 20;
            Criteria criteria;
            algorithms::registration::RegistrationOptimizationParams optimization;
            algorithms::registration::DegenerateRegularizationParams degenerate_regularization;
            algorithms::registration::MapPriorParams map_prior;
        };
        struct Pipeline {
            algorithms::registration::RegistrationRobustScheduleParams robust;
            algorithms::registration::RegistrationVelocityUpdateParams velocity_update;
        };
        Registration registration;
        Pipeline pipeline;
    };

    MotionPrediction motion_prediction;
    LO lo;

    /// lidar_odometry_params.hpp:38-50
    algorithms::registration::RegistrationPipelineParams make_registration_pipeline_params() const {
        algorithms::registration::RegistrationPipelineParams result;
        result.registration = algorithms::registration::RegistrationParams(registration.factor, lo.registration.optimization);
        result.registration.max_iterations = lo.registration.max_iterations;
        result.registration.criteria = lo.registration.criteria;
        result.registration.degenerate_reg = lo.registration.degenerate_regularization;
        result.registration.map_prior = lo.registration.map_prior;
        result.random_sampling = registration_sampling;
        result.robust = lo.pipeline.robust;
        result.velocity_update = lo.pipeline.velocity_update;
        return result;
    }
};

}  // namespace lidar_odometry

// ------------------------------------------------------------------------------------------------ scan processing
namespace pointcloud_processing {

/// pipeline/pointcloud_processing.hpp:25-28 — what prepare_context builds and compute_covariances / refine_filter consume
struct ProcessingContext {
    algorithms::knn::KDTree::Ptr tree;
    algorithms::knn::KNNResult knn_result;
};

/// pipeline/pointcloud_processing.hpp:30-204
class PCProcessor {
public:
    using Ptr = std::shared_ptr<PCProcessor>;
    using ConstPtr = std::shared_ptr<const PCProcessor>;

    PCProcessor(const sycl_utils::DeviceQueue& q, const odometry::CommonParameters::Scan& scan_params,
                const odometry::CommonParameters::CovarianceEstimation& covs_params,
                const odometry::CommonParameters::IMU& imu_params)
        : queue_(q), scan_params_(scan_params), covs_params_(covs_params), imu_params_(imu_params) {
        // :87-101
        preprocess_filter_ = std::make_shared<algorithms::filter::PreprocessFilter>(queue_);
        if (scan_params_.downsampling.voxel.enable)
            voxel_filter_ = std::make_shared<algorithms::filter::VoxelGrid>(queue_, scan_params_.downsampling.voxel.size);
        if (scan_params_.downsampling.polar.enable)
            polar_filter_ = std::make_shared<algorithms::filter::PolarGrid>(
                queue_, scan_params_.downsampling.polar.distance_size, scan_params_.downsampling.polar.elevation_size,
                scan_params_.downsampling.polar.azimuth_size,
                algorithms::coordinate_system_from_string(scan_params_.downsampling.polar.coord_system));
    }

    /// :42-46 — with the configured bias, starting at rest
    template <imu::imu_measurement_range Range>
    void deskew_with_imu(const PointCloudShared& src, PointCloudShared& dst, const Range& imu_buffer,
                         const Eigen::Isometry3f& current_pose) const {
        deskew_with_imu_impl(src, dst, imu_buffer, current_pose, imu_params_.bias, Eigen::Vector3f::Zero());
    }
    /// :48-53
    template <imu::imu_measurement_range Range>
    void deskew_with_imu(const PointCloudShared& src, PointCloudShared& dst, const Range& imu_buffer,
                         const Eigen::Isometry3f& current_pose, const imu::IMUBias& bias,
                         const Eigen::Vector3f& v_world_body_i = Eigen::Vector3f::Zero()) const {
        deskew_with_imu_impl(src, dst, imu_buffer, current_pose, bias, v_world_body_i);
    }

    /// :114-142 — box filter -> polar grid -> voxel grid -> random sampling. `input` tracks where the current data lives; the
    /// grids work in place; when nothing ran dst shares src's containers.
    void prefilter(const PointCloudShared& src, PointCloudShared& dst) const {
        const PointCloudShared* input = &src;
        if (scan_params_.preprocess.box_filter.enable) {
            preprocess_filter_->box_filter(src, dst, scan_params_.preprocess.box_filter.min, scan_params_.preprocess.box_filter.max);
            input = &dst;
        }
        if (scan_params_.downsampling.polar.enable) {
            polar_filter_->downsampling(*input, dst);
            input = &dst;
        }
        if (scan_params_.downsampling.voxel.enable) {
            voxel_filter_->downsampling(*input, dst);
            input = &dst;
        }
        if (input != &dst) dst = src;
        if (scan_params_.downsampling.random.enable) preprocess_filter_->random_sampling(dst, scan_params_.downsampling.random.num);
    }

    void random_sampling(const PointCloudShared& src, PointCloudShared& dst, size_t num) const {
        preprocess_filter_->random_sampling(src, dst, num);
    }

    /// :62-66
    ProcessingContext prepare_context(const PointCloudShared& scan) const {
        ProcessingContext ctx;
        ctx.tree = algorithms::knn::KDTree::build(queue_, scan);
        return ctx;
    }

    /// :144-156 — one kNN search, then the M-estimated or the plain covariances
    void compute_covariances(PointCloudShared& scan, ProcessingContext& ctx) const {
        auto events = ctx.tree->knn_search_async(scan, covs_params_.neighbor_num, ctx.knn_result);
        if (covs_params_.m_estimation.enable)
            events += algorithms::covariance::estimate_robust_async(ctx.knn_result, scan, covs_params_.m_estimation.type,
                                                                    covs_params_.m_estimation.mad_scale,
                                                                    covs_params_.m_estimation.min_robust_scale,
                                                                    covs_params_.m_estimation.max_iterations, events.evs);
        else
            events += algorithms::covariance::estimate_async(ctx.knn_result, scan, events.evs);
        events.wait_and_throw();
    }

    /// :158-203 — angle of incidence, intensity correction, Gaussian smoothing, local-mean normalisation; the two neighbourhood
    /// filters reuse the covariance search when it has neighbours enough and search again otherwise
    void refine_filter(PointCloudShared& scan, const ProcessingContext& ctx) const {
        namespace alg = algorithms;
        if (scan_params_.preprocess.angle_incidence_filter.enable)
            preprocess_filter_->angle_incidence_filter(scan, scan, scan_params_.preprocess.angle_incidence_filter.min_angle,
                                                       scan_params_.preprocess.angle_incidence_filter.max_angle);
        if (scan_params_.intensity_correction.enable && !scan_params_.enhanced_reflectivity.enable && scan.has_intensity()) {
            const auto& ic = scan_params_.intensity_correction;
            alg::intensity_correction::correct_intensity(scan, ic.exp, ic.scale, ic.min_intensity, ic.max_intensity, ic.ref_distance,
                                                         ic.angle_exponent);
        }
        if (scan_params_.intensity_gaussian.enable && scan.has_intensity()) {
            const auto& gp = scan_params_.intensity_gaussian;
            if (gp.neighbor_num <= ctx.knn_result.k) {
                alg::intensity_gaussian::smooth_intensity(scan, ctx.knn_result, gp.sigma_azimuth, gp.sigma_elevation, gp.sigma_range,
                                                          gp.neighbor_num);
            } else {
                const auto gaussian_knn = context_tree(ctx, "intensity_gaussian").knn_search(scan, gp.neighbor_num);
                alg::intensity_gaussian::smooth_intensity(scan, gaussian_knn, gp.sigma_azimuth, gp.sigma_elevation, gp.sigma_range);
            }
        }
        if (scan_params_.intensity_local_mean_norm.enable && scan.has_intensity()) {
            const auto& lp = scan_params_.intensity_local_mean_norm;
            if (lp.neighbor_num <= ctx.knn_result.k) {
                alg::intensity_local_mean_norm::normalize(scan, ctx.knn_result, lp.sigma_azimuth, lp.sigma_elevation, lp.sigma_range,
                                                          lp.mean_min, lp.neighbor_num);
            } else {
                const auto local_knn = context_tree(ctx, "intensity_local_mean_norm").knn_search(scan, lp.neighbor_num);
                alg::intensity_local_mean_norm::normalize(scan, local_knn, lp.sigma_azimuth, lp.sigma_elevation, lp.sigma_range,
                                                          lp.mean_min);
            }
        }
    }

private:
    /// (the reference dereferences ctx.tree here; a context nobody prepared is reported instead)
    static const algorithms::knn::KDTree& context_tree(const ProcessingContext& ctx, const char* who) {
        if (ctx.tree == nullptr)
            throw std::runtime_error(std::string("[PCProcessor::refine_filter] ") + who + " needs a prepared context (prepare_context)");
        return *ctx.tree;
    }
    /// :103-112
    template <imu::imu_measurement_range Range>
    void deskew_with_imu_impl(const PointCloudShared& src, PointCloudShared& dst, const Range& imu_buffer,
                              const Eigen::Isometry3f& current_pose, const imu::IMUBias& bias,
                              const Eigen::Vector3f& v_world_body_i) const {
        const double scan_start_sec = src.start_time_ms * 1e-3;
        const Eigen::Matrix3f R_world_imu =
            sycl_points::detail::rotation_of(current_pose) * sycl_points::detail::rotation_of(imu_params_.T_imu_to_lidar);
        algorithms::deskew::deskew_point_cloud_imu(src, dst, imu_buffer, scan_start_sec, imu_params_.T_imu_to_lidar, bias,
                                                   imu_params_.preintegration, R_world_imu, v_world_body_i, nullptr,
                                                   imu_params_.deskew.gyro_only);
    }

    sycl_utils::DeviceQueue queue_;
    algorithms::filter::PreprocessFilter::Ptr preprocess_filter_ = nullptr;
    algorithms::filter::VoxelGrid::Ptr voxel_filter_ = nullptr;
    algorithms::filter::PolarGrid::Ptr polar_filter_ = nullptr;
    odometry::CommonParameters::Scan scan_params_;
    odometry::CommonParameters::CovarianceEstimation covs_params_;
    odometry::CommonParameters::IMU imu_params_;
};

}  // namespace pointcloud_processing

// ------------------------------------------------------------------------------------------------ submap
namespace submapping {

/// pipeline/submapping.hpp:18-248 — the registration target: an occupancy grid fed with every accepted frame, or a voxel hash map
/// fed with keyframes
class Submap {
public:
    using Ptr = std::shared_ptr<Submap>;
    using ConstPtr = std::shared_ptr<const Submap>;
    using OdometryCommonParams = odometry::CommonParameters;
    using SubmapMapType = odometry::SubmapMapType;

    const auto& get_last_keyframe_pose() const { return last_keyframe_pose_; }
    const auto& get_keyframe_poses() const { return keyframe_poses_; }
    const auto& get_submap_kdtree() const { return *submap_tree_; }
    const PointCloudShared& get_submap_point_cloud() const { return *submap_pc_ptr_; }
    const PointCloudShared& get_last_keyframe_point_cloud() const { return *last_keyframe_pc_; }

    /// :32-76
    Submap(const sycl_utils::DeviceQueue& queue, const OdometryCommonParams& params) : queue_(queue) {
        last_keyframe_pc_ = std::make_shared<PointCloudShared>(queue_);
        submap_pc_ptr_ = std::make_shared<PointCloudShared>(queue_);
        submap_pc_tmp_ = std::make_shared<PointCloudShared>(queue_);
        submap_params_ = params.submap;
        cov_params_ = params.covariance_estimation;
        reg_params_ = params.registration;
        last_keyframe_pose_ = params.pose.initial;
        last_keyframe_time_ = -1.0;
        keyframe_poses_.clear();
        keyframe_poses_.push_back(params.pose.initial);
        preprocess_filter_ = std::make_shared<algorithms::filter::PreprocessFilter>(queue_);
        if (submap_params_.map_type == SubmapMapType::OCCUPANCY_GRID_MAP) {
            const auto& og = submap_params_.occupancy_grid_map;
            occupancy_grid_ = std::make_shared<algorithms::mapping::OccupancyGridMap>(queue_, submap_params_.voxel_size);
            occupancy_grid_->set_log_odds_hit(og.log_odds_hit);
            occupancy_grid_->set_log_odds_miss(og.log_odds_miss);
            occupancy_grid_->set_log_odds_limits(og.log_odds_limits_min, og.log_odds_limits_max);
            occupancy_grid_->set_occupancy_threshold(og.occupied_threshold);
            occupancy_grid_->set_free_space_updates_enabled(og.enable_free_space_updates);
            occupancy_grid_->set_voxel_pruning_enabled(og.enable_pruning);
            occupancy_grid_->set_stale_frame_threshold(static_cast<uint32_t>(og.stale_frame_threshold));
        } else {
            submap_voxel_ = std::make_shared<algorithms::mapping::VoxelHashMap>(queue_, submap_params_.voxel_size);
        }
    }

    /// :85-94 — the first keyframe, anchored at the pipeline's current pose
    void add_first_frame(const PointCloudShared& cloud, double timestamp, const Eigen::Isometry3f& current_pose) {
        last_keyframe_pose_ = current_pose;
        if (keyframe_poses_.empty()) keyframe_poses_.push_back(current_pose);
        else keyframe_poses_.front() = current_pose;
        build_submap(cloud, current_pose, true);
        last_keyframe_time_ = timestamp;
    }

    /// :96-121 — false: the registration is taken as failed (inlier ratio), or the voxel map saw no keyframe
    bool add_frame(const PointCloudShared& preprocessed_cloud, const algorithms::registration::RegistrationResult& reg_result,
                   float inlier_ratio, double timestamp, shared_vector_ptr<float> random_sampling_weights = nullptr) {
        if (submap_params_.keyframe.inlier_ratio_threshold > 0.0f && inlier_ratio <= submap_params_.keyframe.inlier_ratio_threshold)
            return false;
        if (submap_params_.map_type == SubmapMapType::OCCUPANCY_GRID_MAP) {
            build_submap(preprocessed_cloud, reg_result.T, false, random_sampling_weights);
            return true;
        }
        if (is_keyframe(reg_result, timestamp)) {
            last_keyframe_pose_ = reg_result.T;
            last_keyframe_time_ = timestamp;
            keyframe_poses_.push_back(reg_result.T);
            build_submap(preprocessed_cloud, reg_result.T, false, random_sampling_weights);
            return true;
        }
        return false;
    }

private:
    /// :144-161 (sp_keyframe_decision_host)
    bool is_keyframe(const algorithms::registration::RegistrationResult& reg_result, double timestamp) const {
        int flag = 0;
        const TransformMatrix last = last_keyframe_pose_.matrix(), cur = reg_result.T.matrix();
        throw_on_error(sp_keyframe_decision_host(last.data(), cur.data(), last_keyframe_time_, timestamp,
                                                 submap_params_.keyframe.distance_threshold,
                                                 submap_params_.keyframe.angle_threshold_degrees,
                                                 submap_params_.keyframe.time_threshold_seconds, &flag, nullptr));
        return flag != 0;
    }

    /// :163-201
    void build_submap(const PointCloudShared& cloud, const Eigen::Isometry3f& current_pose, bool is_first_frame,
                      shared_vector_ptr<float> random_sampling_weights = nullptr) {
        if (random_sampling_weights && random_sampling_weights->size() == cloud.size())
            preprocess_filter_->mixed_random_sampling(cloud, *last_keyframe_pc_, *random_sampling_weights,
                                                      submap_params_.point_random_sampling_num, submap_params_.weighted_sampling_ratio);
        else
            preprocess_filter_->random_sampling(cloud, *last_keyframe_pc_, submap_params_.point_random_sampling_num);
        if (submap_params_.map_type == SubmapMapType::OCCUPANCY_GRID_MAP) {
            occupancy_grid_->add_point_cloud(*last_keyframe_pc_, current_pose);
            occupancy_grid_->extract_occupied_points(*submap_pc_tmp_, current_pose, submap_params_.max_distance_range);
        } else {
            submap_voxel_->add_point_cloud(*last_keyframe_pc_, current_pose);
            submap_voxel_->downsampling(*submap_pc_tmp_, current_pose.translation(), submap_params_.max_distance_range);
        }
        if (is_first_frame)
            *submap_pc_ptr_ = algorithms::transform::transform_copy(cloud, current_pose.matrix());
        else if (submap_pc_tmp_->size() >= reg_params_.min_num_points)
            std::swap(submap_pc_ptr_, submap_pc_tmp_);
        submap_tree_ = algorithms::knn::KDTree::build(queue_, *submap_pc_ptr_);
        compute_covariances();
    }

    /// :203-247 — what the factor needs and the submap lacks, over one lazily launched kNN search
    void compute_covariances() {
        namespace reg = algorithms::registration;
        bool knn_ready = false;
        sycl_utils::events knn_events;
        auto ensure_knn = [&]() {
            if (!knn_ready) {
                knn_events = submap_tree_->knn_search_async(*submap_pc_ptr_, cov_params_.neighbor_num, knn_result_);
                knn_ready = true;
            }
        };
        sycl_utils::events cov_events;
        const auto reg_type = reg_params_.factor.reg_type;
        const bool need_covariances = reg_type == reg::RegType::GICP || reg_type == reg::RegType::POINT_TO_DISTRIBUTION ||
                                      reg_type == reg::RegType::GENZ || reg_params_.factor.rotation_constraint.enable;
        const bool need_normals = reg_type == reg::RegType::POINT_TO_PLANE || reg_type == reg::RegType::GENZ;
        const bool submap_has_cov = submap_pc_ptr_->has_cov();
        if (need_normals) {
            ensure_knn();
            if (submap_has_cov) cov_events += algorithms::covariance::extract_normals_async(*submap_pc_ptr_, knn_events.evs);
            else cov_events += algorithms::covariance::estimate_normals_async(knn_result_, *submap_pc_ptr_, knn_events.evs);
        }
        if (need_covariances && !submap_has_cov) {
            ensure_knn();
            cov_events += algorithms::covariance::estimate_async(knn_result_, *submap_pc_ptr_, knn_events.evs);
        }
        cov_events.wait_and_throw();
    }

    sycl_utils::DeviceQueue queue_;
    OdometryCommonParams::Submap submap_params_;
    OdometryCommonParams::CovarianceEstimation cov_params_;
    OdometryCommonParams::Registration reg_params_;
    algorithms::knn::KNNResult knn_result_;
    double last_keyframe_time_;             // [s]
    Eigen::Isometry3f last_keyframe_pose_;  // keyframe T_odom_to_lidar
    std::vector<Eigen::Isometry3f, Eigen::aligned_allocator<Eigen::Isometry3f>> keyframe_poses_;
    algorithms::filter::PreprocessFilter::Ptr preprocess_filter_ = nullptr;
    algorithms::mapping::VoxelHashMap::Ptr submap_voxel_ = nullptr;
    algorithms::mapping::OccupancyGridMap::Ptr occupancy_grid_ = nullptr;
    algorithms::knn::KDTree::Ptr submap_tree_ = nullptr;
    PointCloudShared::Ptr last_keyframe_pc_ = nullptr;  // sensor frame
    PointCloudShared::Ptr submap_pc_ptr_ = nullptr;     // odom / world frame
    PointCloudShared::Ptr submap_pc_tmp_ = nullptr;     // odom / world frame
};

}  // namespace submapping

// ------------------------------------------------------------------------------------------------ what the two loops share
namespace odometry {

/// What pipeline/lidar_odometry.hpp and pipeline/lidar_inertial_odometry.hpp each hold, word for word: the IMU buffer with its mutex
/// and rules, the timing maps, a stage's exception as an error result, the three conditions of the scan covariances and the
/// constructor's widening of the IMU buffer. The two differ in the stderr prefix and in the name of stage 3 only.
class PipelineCommon {
public:
    const auto& get_error_message() const { return error_message_; }
    const auto& get_current_processing_time() const { return current_processing_time_; }
    const auto& get_total_processing_times() const { return total_processing_times_; }

    /// lidar_odometry.hpp:85-106, lidar_inertial_odometry.hpp:112-121 — no-op with the IMU disabled; non-finite samples and stamps
    /// that do not increase are dropped; the buffer is cut to buffer_duration_sec. May be called while process() runs.
    void add_imu_measurement(const imu::IMUMeasurement& meas) {
        if (!imu_enabled_) return;
        std::lock_guard<std::mutex> lock(imu_mutex_);
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(meas.accel[k]) || !std::isfinite(meas.gyro[k])) return;
        if (!imu_buffer_.empty() && meas.timestamp <= imu_buffer_.back().timestamp) return;
        const double latest_timestamp = meas.timestamp;
        imu_buffer_.push_back(meas);
        while (latest_timestamp - imu_buffer_.front().timestamp > imu_buffer_duration_sec_) imu_buffer_.pop_front();
    }

    /// lidar_odometry.hpp:110-113, lidar_inertial_odometry.hpp:123-126 — a snapshot
    std::deque<imu::IMUMeasurement> get_imu_buffer() const {
        std::lock_guard<std::mutex> lock(imu_mutex_);
        return imu_buffer_;
    }

protected:
    PipelineCommon(const char* log_prefix, const char* registration_stage)
        : log_prefix_(log_prefix), registration_stage_(registration_stage) {}

    /// lidar_odometry.hpp:41-52, lidar_inertial_odometry.hpp:73-80 — the IMU buffer must outlast the alignment window (the trimming
    /// keeps span <= buffer_duration_sec); the rules add_imu_measurement applies are those of the widened parameters
    void adopt_imu_params(CommonParameters::IMU& imu) {
        if (imu.enable && imu.initial_alignment.enable) {
            const double need = static_cast<double>(imu.initial_alignment.required_duration_sec) + 0.2;
            if (imu.buffer_duration_sec < need) imu.buffer_duration_sec = need;
        }
        imu_enabled_ = imu.enable;
        imu_buffer_duration_sec_ = imu.buffer_duration_sec;
    }

    enum class ProcessName { preprocessing = 0, compute_covariances, registration, build_submap };
    const char* process_name(ProcessName n) const {  // lidar_odometry.hpp:357-362, lidar_inertial_odometry.hpp:339-344
        switch (n) {
            case ProcessName::preprocessing: return "1. preprocessing";
            case ProcessName::compute_covariances: return "2. compute covariances";
            case ProcessName::registration: return registration_stage_;
            case ProcessName::build_submap: return "4. build submap";
        }
        return "";
    }
    void clear_current_processing_time() {
        current_processing_time_.clear();
        for (ProcessName n : {ProcessName::preprocessing, ProcessName::compute_covariances, ProcessName::registration, ProcessName::build_submap})
            current_processing_time_[process_name(n)] = 0.0;
    }
    void clear_total_processing_times() {
        total_processing_times_.clear();
        for (ProcessName n : {ProcessName::preprocessing, ProcessName::compute_covariances, ProcessName::registration, ProcessName::build_submap})
            total_processing_times_[process_name(n)] = {};
    }
    void add_delta_time(ProcessName name, double dt) {
        total_processing_times_[process_name(name)].push_back(dt);
        current_processing_time_[process_name(name)] = dt;
    }
    /// a stage's exception becomes ResultType::error with "<stage>: <what>" (lidar_odometry.hpp:145-151 and its siblings)
    template <class F>
    bool run_stage(const char* stage, F&& f) {
        try {
            f();
            return true;
        } catch (const std::exception& e) {
            error_message_ = std::string(stage) + ": " + e.what();
            std::cerr << log_prefix_ << " " << error_message_ << std::endl;
            return false;
        }
    }

    /// lidar_odometry.hpp:508-522, lidar_inertial_odometry.hpp:646-660 — only when the factor, the incidence filter or an intensity
    /// filter needs them
    static void compute_covariances(const CommonParameters& params, const pointcloud_processing::PCProcessor& pc_processor,
                                    PointCloudShared& preprocessed_pc, pointcloud_processing::ProcessingContext& processing_ctx) {
        namespace reg = algorithms::registration;
        const bool needs_covs = params.registration.factor.reg_type == reg::RegType::GICP ||
                                params.registration.factor.rotation_constraint.enable ||
                                params.scan.preprocess.angle_incidence_filter.enable;
        const bool needs_gaussian = params.scan.intensity_gaussian.enable && preprocessed_pc.has_intensity();
        const bool needs_local_mean_norm = params.scan.intensity_local_mean_norm.enable && preprocessed_pc.has_intensity();
        if (!needs_covs && !needs_gaussian && !needs_local_mean_norm) return;
        processing_ctx = pc_processor.prepare_context(preprocessed_pc);
        pc_processor.compute_covariances(preprocessed_pc, processing_ctx);
    }

    std::deque<imu::IMUMeasurement> imu_buffer_;
    mutable std::mutex imu_mutex_;  // guards imu_buffer_ (written by the IMU callback, read by the LiDAR callback)
    std::string error_message_;
    std::map<std::string, double> current_processing_time_;
    std::map<std::string, std::vector<double>> total_processing_times_;

private:
    const char* log_prefix_;
    const char* registration_stage_;
    bool imu_enabled_ = false;
    double imu_buffer_duration_sec_ = 0.0;
};

}  // namespace odometry

// ------------------------------------------------------------------------------------------------ the odometry loop
namespace lidar_odometry {
using LidarOdometryParams = lidar_odometry::Parameters;

/// pipeline/lidar_odometry.hpp:27-622 — what the reference's ROS 2 node calls once per scan
class LiDAROdometryPipeline : public odometry::PipelineCommon {
public:
    using Ptr = std::shared_ptr<LiDAROdometryPipeline>;
    using ConstPtr = std::shared_ptr<const LiDAROdometryPipeline>;

    enum class ResultType : std::int8_t {
        success = 0,
        first_frame,
        waiting_initial_alignment,
        error = 100,
        old_timestamp,
        small_number_of_points
    };

    /// :41-52 — the IMU buffer must outlast the alignment window (the trimming keeps span <= buffer_duration_sec)
    LiDAROdometryPipeline(const LidarOdometryParams& params) : PipelineCommon("[LiDAR Odometry]", "3. registration") {
        params_ = params;
        adopt_imu_params(params_.imu);
        initialize();
    }

    auto get_device_queue() const { return queue_ptr_; }
    /// current / previous LiDAR pose in the (gravity-aligned) odom frame
    const auto& get_odom() const { return odom_; }
    const auto& get_prev_odom() const { return prev_odom_; }
    const auto& get_last_keyframe_pose() const { return submap_->get_last_keyframe_pose(); }
    const auto& get_keyframe_poses() const { return submap_->get_keyframe_poses(); }
    const PointCloudShared& get_preprocessed_point_cloud() const { return *preprocessed_pc_; }
    const PointCloudShared& get_submap_point_cloud() const { return submap_->get_submap_point_cloud(); }
    const PointCloudShared& get_last_keyframe_point_cloud() const { return submap_->get_last_keyframe_point_cloud(); }
    const PointCloudShared* get_registration_input_point_cloud() const {
        return registration_pipeline_->get_registration_input_point_cloud();
    }
    const auto& get_registration_result() const { return *reg_result_; }
    /// MI355X extension: the parameters as the constructor adjusted them (buffer_duration_sec, velocity_update.enable)
    const LidarOdometryParams& get_params() const { return params_; }

    /// :115-298
    ResultType process(const PointCloudShared::Ptr scan, double timestamp) {
        error_message_.clear();
        // initial roll / pitch from stationary IMU samples, once, before the first scan becomes the reference frame (:121-129)
        if (is_first_frame_ && alignment_estimator_ && alignment_estimator_->enabled() && !alignment_estimator_->is_done()) {
            const auto out = alignment_estimator_->try_align(timestamp, get_imu_buffer(), imu_bias_);
            if (out.status != imu::InitialAlignmentEstimator::Status::success) {
                error_message_ = std::string("initial_alignment: ") + out.error_message;
                return ResultType::waiting_initial_alignment;
            }
            apply_initial_alignment(out);
        }
        if (last_frame_time_ > 0.0) {  // :131-139
            const float dt = static_cast<float>(timestamp - last_frame_time_);
            if (dt > 0.0f) {
                dt_ = dt;
            } else {
                error_message_ = "old timestamp";
                return ResultType::old_timestamp;
            }
        }
        clear_current_processing_time();

        double dt_preprocessing = 0.0;
        if (!run_stage("preprocess", [&]() { time_utils::measure_execution([&]() { preprocess(scan); }, dt_preprocessing); }))
            return ResultType::error;
        {
            double dt_covariance = 0.0;
            if (!run_stage("compute_covariances", [&]() { time_utils::measure_execution([&]() { compute_covariances(); }, dt_covariance); }))
                return ResultType::error;
            add_delta_time(ProcessName::compute_covariances, dt_covariance);
        }
        {
            double dt_refine_filter = 0.0;
            if (!run_stage("refine_filter", [&]() {
                    time_utils::measure_execution([&]() { pc_processor_->refine_filter(*preprocessed_pc_, processing_ctx_); }, dt_refine_filter);
                }))
                return ResultType::error;
            dt_preprocessing += dt_refine_filter;
            add_delta_time(ProcessName::preprocessing, dt_preprocessing);
        }
        if (preprocessed_pc_->size() <= params_.registration.min_num_points) {  // :182-185
            error_message_ = "point cloud size is too small";
            return ResultType::small_number_of_points;
        }

        if (is_first_frame_) {  // :188-220 — anchored at odom_ (post-alignment), so later frames share its frame
            if (!run_stage("build_submap (first frame)", [&]() { submap_->add_first_frame(*preprocessed_pc_, timestamp, odom_); }))
                return ResultType::error;
            is_first_frame_ = false;
            last_frame_time_ = timestamp;
            if (imu_preintegration_) {
                const Eigen::Matrix3f R_world_imu =
                    sycl_points::detail::rotation_of(odom_) * sycl_points::detail::rotation_of(params_.imu.T_imu_to_lidar);
                std::lock_guard<std::mutex> lock(imu_mutex_);
                imu_preintegration_->reset(imu_bias_, Eigen::Matrix<float, 15, 15>::Zero(), R_world_imu);
                imu_R_world_at_reset_ = R_world_imu;
                imu_v_world_at_reset_ = Eigen::Vector3f::Zero();
                last_imu_reset_timestamp_ = timestamp;
            }
            return ResultType::first_frame;
        }

        if (imu_preintegration_) {  // :223-238 — the IMU window [last reset, timestamp]
            imu_batch_.clear();
            {
                std::lock_guard<std::mutex> lock(imu_mutex_);
                imu_batch_.reserve(imu_buffer_.size());
                imu::build_measurement_window(imu_buffer_, last_imu_reset_timestamp_, timestamp, imu_batch_);
            }
            constexpr double kTimestampToleranceSec = 1e-6;
            imu_window_complete_ = imu_batch_.size() >= 2 &&
                                   std::abs(imu_batch_.front().timestamp - last_imu_reset_timestamp_) <= kTimestampToleranceSec &&
                                   std::abs(imu_batch_.back().timestamp - timestamp) <= kTimestampToleranceSec;
            imu_preintegration_->integrate_batch(imu_batch_);
        }

        {
            double dt_registration = 0.0;
            if (!run_stage("registration", [&]() {
                    *reg_result_ = time_utils::measure_execution([&]() { return registration(); }, dt_registration);
                }))
                return ResultType::error;
            add_delta_time(ProcessName::registration, dt_registration);
        }
        last_imu_reset_timestamp_ = timestamp;

        {
            double dt_build_submap = 0.0;
            if (!run_stage("submapping", [&]() {
                    time_utils::measure_execution([&]() { submapping(*reg_result_, timestamp); }, dt_build_submap);
                }))
                return ResultType::error;
            add_delta_time(ProcessName::build_submap, dt_build_submap);
        }

        // the full-resolution cloud that is published follows the registered motion too (:270-274)
        if (params_.lo.pipeline.velocity_update.enable && !is_imu_deskew_enabled())
            algorithms::deskew::deskew_point_cloud_constant_velocity(*preprocessed_pc_, *preprocessed_pc_, odom_, reg_result_->T, dt_);

        {  // :277-296
            prev_odom_ = odom_;
            odom_ = reg_result_->T;
            last_frame_time_ = timestamp;
            float aa[4];
            const TransformMatrix prev = prev_odom_.matrix(), cur = odom_.matrix();
            throw_on_error(sp_velocity_from_poses_host(prev.data(), cur.data(), dt_, linear_velocity_.data(), aa));
            angular_velocity_ = Eigen::AngleAxisf(aa[0], Eigen::Vector3f(aa[1], aa[2], aa[3]));
            if (imu_preintegration_ && params_.motion_prediction.mode == MotionPredictionMode::IMU_SE3) {
                const Eigen::Matrix3f R_world_imu_prev =
                    sycl_points::detail::rotation_of(prev_odom_) * sycl_points::detail::rotation_of(params_.imu.T_imu_to_lidar);
                imu_velocity_corrector_.update(odom_.translation() - prev_odom_.translation(), R_world_imu_prev,
                                               params_.imu.preintegration.gravity);
            }
            registrated_ = true;
        }
        return ResultType::success;
    }

private:
    bool is_imu_deskew_enabled() const { return params_.imu.enable && params_.imu.deskew.enable; }

    /// :387-474
    void initialize() {
        queue_ptr_ = std::make_shared<sycl_utils::DeviceQueue>(0);  // (params_.device is not consulted)
        icp_weights_ = std::make_shared<shared_vector<float>>(*queue_ptr_);
        preprocessed_pc_ = std::make_shared<PointCloudShared>(*queue_ptr_);
        odom_ = params_.pose.initial;
        prev_odom_ = params_.pose.initial;
        linear_velocity_ = Eigen::Vector3f::Zero();
        angular_velocity_ = Eigen::AngleAxisf::Identity();
        pc_processor_ = std::make_shared<pointcloud_processing::PCProcessor>(*queue_ptr_, params_.scan, params_.covariance_estimation,
                                                                             params_.imu);
        submap_ = std::make_shared<submapping::Submap>(*queue_ptr_, params_);
        {
            auto reg_pipeline_params = params_.make_registration_pipeline_params();
            if (is_imu_deskew_enabled() && reg_pipeline_params.velocity_update.enable) {
                std::cerr << "[LiDAR Odometry] VelocityUpdate is disabled because IMU deskew is enabled." << std::endl;
                reg_pipeline_params.velocity_update.enable = false;
                params_.lo.pipeline.velocity_update.enable = false;
            }
            registration_pipeline_ = std::make_shared<algorithms::registration::RegistrationPipeline>(*queue_ptr_, reg_pipeline_params);
            reg_result_ = std::make_shared<algorithms::registration::RegistrationResult>();
            registrated_ = false;
        }
        clear_total_processing_times();
        motion_predictor_ = std::make_shared<MotionPredictor>(params_.motion_prediction);
        if (!params_.imu.enable && params_.motion_prediction.mode == MotionPredictionMode::GYRO_LIDAR_CV)
            std::cerr << "[LiDAR Odometry] " << MotionPredictionMode_to_string(params_.motion_prediction.mode)
                      << " requires IMU; falling back to LIDAR_CV." << std::endl;
        imu_bias_ = params_.imu.bias;
        if (params_.imu.enable && params_.motion_prediction.mode != MotionPredictionMode::LIDAR_CV) {
            imu_preintegration_ = std::make_shared<imu::IMUPreintegration>(params_.imu.preintegration);
            const Eigen::Matrix3f R_world_imu =
                sycl_points::detail::rotation_of(params_.pose.initial) * sycl_points::detail::rotation_of(params_.imu.T_imu_to_lidar);
            imu_preintegration_->reset(imu_bias_, Eigen::Matrix<float, 15, 15>::Zero(), R_world_imu);
            imu_R_world_at_reset_ = R_world_imu;
            imu_v_world_at_reset_ = Eigen::Vector3f::Zero();
        }
        if (params_.imu.enable)
            alignment_estimator_ = std::make_shared<imu::InitialAlignmentEstimator>(
                params_.imu.initial_alignment, params_.imu.preintegration.gravity, params_.imu.T_imu_to_lidar);
    }

    /// :487-494 — the gravity-corrected rotation with the user's yaw layered on the left; the gyro bias the alignment found
    void apply_initial_alignment(const imu::InitialAlignmentEstimator::Output& out) {
        const float yaw_user = imu::detail::yaw_from_rotation(sycl_points::detail::rotation_of(params_.pose.initial));
        const Eigen::Matrix3f R_odom_lidar =
            Eigen::AngleAxisf(yaw_user, Eigen::Vector3f(0.0f, 0.0f, 1.0f)).toRotationMatrix() * out.R_gravity_lidar;
        sycl_points::detail::set_rotation(odom_, R_odom_lidar);
        sycl_points::detail::set_rotation(prev_odom_, R_odom_lidar);
        imu_bias_.gyro_bias = out.gyro_bias;
    }

    /// :496-502
    void preprocess(const PointCloudShared::Ptr scan) {
        if (is_imu_deskew_enabled()) {
            auto imu_buf_snapshot = get_imu_buffer();
            pc_processor_->deskew_with_imu(*scan, *scan, imu_buf_snapshot, odom_);
        }
        pc_processor_->prefilter(*scan, *preprocessed_pc_);
    }

    /// :508-522
    void compute_covariances() { PipelineCommon::compute_covariances(params_, *pc_processor_, *preprocessed_pc_, processing_ctx_); }

    /// :526-542 — odom * (T_imu_to_lidar * T_imu_rel * T_imu_to_lidar^-1)
    Eigen::Isometry3f imu_motion_prediction() {
        const TransformMatrix T_imu_rel =
            imu_preintegration_->predict_relative_transform(imu_R_world_at_reset_, imu_v_world_at_reset_, imu_bias_);
        const Eigen::Isometry3f& T_i2l = params_.imu.T_imu_to_lidar;
        return odom_ * (T_i2l * sycl_points::detail::isometry_of(T_imu_rel) * T_i2l.inverse());
    }

    /// :544-597
    algorithms::registration::RegistrationResult registration() {
        Eigen::Vector3f v_reset = Eigen::Vector3f::Zero();
        const bool has_imu_prediction = imu_preintegration_ && imu_window_complete_ && imu_preintegration_->get_dt_total() > 0.0;
        MotionPredictionCandidates candidates;
        if (has_imu_prediction) {
            const Eigen::Matrix3f delta_R_imu = imu_preintegration_->get_corrected(imu_bias_).Delta_R;
            const Eigen::Matrix3f R_i2l = sycl_points::detail::rotation_of(params_.imu.T_imu_to_lidar);
            candidates.gyro_delta_rotation_lidar = R_i2l * delta_R_imu * R_i2l.transpose();
            if (params_.motion_prediction.mode == MotionPredictionMode::IMU_SE3) candidates.imu_se3_pose = imu_motion_prediction();
        }
        const Eigen::Isometry3f init_T =
            motion_predictor_->predict(linear_velocity_, angular_velocity_, odom_, dt_, reg_result_, registrated_, candidates);
        if (imu_preintegration_ && params_.motion_prediction.mode == MotionPredictionMode::IMU_SE3)
            // (linear_velocity_ is in the previous LiDAR body frame)
            v_reset = imu_velocity_corrector_.get_reset_velocity(*imu_preintegration_, imu_bias_,
                                                                 sycl_points::detail::rotation_of(prev_odom_) * linear_velocity_);
        // the previous result as a MAP prior: the optimiser stays near init_T where the geometry constrains it weakly
        if (registrated_) registration_pipeline_->registration()->set_map_prior_state(*reg_result_, init_T);

        algorithms::registration::Registration::ExecutionOptions options;
        options.dt = dt_;
        options.prev_pose = odom_.matrix();
        auto result = registration_pipeline_->align(*preprocessed_pc_, submap_->get_submap_point_cloud(), submap_->get_submap_kdtree(),
                                                    init_T.matrix(), options);
        // the next window starts at the pose just registered; the velocity keeps the corrector's value (:583-594)
        if (imu_preintegration_) {
            imu_R_world_at_reset_ = sycl_points::detail::rotation_of(result.T) * sycl_points::detail::rotation_of(params_.imu.T_imu_to_lidar);
            imu_v_world_at_reset_ = v_reset;
            imu_preintegration_->reset(imu_bias_, Eigen::Matrix<float, 15, 15>::Zero(), imu_R_world_at_reset_);
        }
        return result;
    }

    /// :599-621 — robust ICP weights only when the registration cloud is larger than the submap's sample
    void submapping(const algorithms::registration::RegistrationResult& reg_result, double timestamp) {
        const auto reg_pc_ptr = registration_pipeline_->get_deskewed_point_cloud();
        if (reg_pc_ptr == nullptr)
            throw std::runtime_error("[LiDAR Odometry] get_deskewed_point_cloud() returned nullptr unexpectedly.");
        shared_vector_ptr<float> icp_weights = nullptr;
        if (reg_pc_ptr->size() > params_.submap.point_random_sampling_num) {
            const float robust_scale = params_.lo.pipeline.robust.auto_scale ? params_.lo.pipeline.robust.min_scale
                                                                             : params_.registration.factor.robust.default_scale;
            registration_pipeline_->compute_icp_robust_weights(submap_->get_submap_point_cloud(), submap_->get_submap_kdtree(),
                                                               reg_result.T.matrix(), robust_scale, *icp_weights_);
            icp_weights = icp_weights_;
        }
        const float inlier_ratio = registration_pipeline_->get_inlier_ratio(reg_result);
        submap_->add_frame(*reg_pc_ptr, reg_result, inlier_ratio, timestamp, icp_weights);
    }

    sycl_utils::DeviceQueue::Ptr queue_ptr_ = nullptr;
    PointCloudShared::Ptr preprocessed_pc_ = nullptr;  // sensor frame
    bool is_first_frame_ = true;
    pointcloud_processing::ProcessingContext processing_ctx_;
    shared_vector_ptr<float> icp_weights_ = nullptr;
    pointcloud_processing::PCProcessor::Ptr pc_processor_ = nullptr;
    algorithms::registration::RegistrationPipeline::Ptr registration_pipeline_ = nullptr;
    bool registrated_ = false;
    algorithms::registration::RegistrationResult::Ptr reg_result_ = nullptr;
    Eigen::Vector3f linear_velocity_;     // [m/s] in the previous LiDAR body frame
    Eigen::AngleAxisf angular_velocity_;  // [rad/s]
    Eigen::Isometry3f prev_odom_;         // T_odom_to_lidar
    Eigen::Isometry3f odom_;
    submapping::Submap::Ptr submap_ = nullptr;
    double last_frame_time_ = -1.0;  // [s]
    float dt_ = -1.0f;               // [s]
    Parameters params_;
    MotionPredictor::Ptr motion_predictor_ = nullptr;
    imu::IMUPreintegration::Ptr imu_preintegration_ = nullptr;
    imu::IMUVelocityCorrector imu_velocity_corrector_;
    imu::IMUBias imu_bias_;  // params_.imu.bias, then what the initial alignment found
    imu::InitialAlignmentEstimator::Ptr alignment_estimator_ = nullptr;
    double last_imu_reset_timestamp_ = -1.0;  // LiDAR stamp of the last preintegration reset
    Eigen::Matrix3f imu_R_world_at_reset_ = Eigen::Matrix3f::Identity();
    Eigen::Vector3f imu_v_world_at_reset_ = Eigen::Vector3f::Zero();
    std::vector<imu::IMUMeasurement> imu_batch_;
    bool imu_window_complete_ = false;
};

}  // namespace lidar_odometry

// ------------------------------------------------------------------------------------------------ the LiDAR-inertial loop
namespace lidar_inertial_odometry {

/// pipeline/lidar_inertial_odometry_params.hpp:15-57 — the IMU is mandatory: the pipeline forces imu.enable
struct Parameters : public odometry::CommonParameters {
    struct LIO {
        algorithms::lio::LIORegistrationParams registration;

        struct PreintegrationReset {
            float fd_velocity_sigma = 0.1f;    ///< [m/s] floor on the velocity block of the covariance at each IMU reset
            float icp_rotation_sigma = 0.01f;  ///< [rad] the same for the rotation block
        };
        /// safeguards for the weakly observable bias states
        struct BiasEstimation {
            bool freeze_on_low_excitation = false;    ///< hold the biases while the window shows no excitation
            float gyro_excitation_threshold = 0.03f;  ///< [rad/s] max |w - mean w| above which the gyro counts as excited
            float accel_excitation_threshold = 0.3f;  ///< [m/s^2] the same for the specific force
            float max_accel_bias = 0.0f;              ///< [m/s^2] clamp on the bias norm; <= 0 disables
            float max_gyro_bias = 0.0f;               ///< [rad/s]
        };
        PreintegrationReset preintegration_reset;
        BiasEstimation bias_estimation;
    };

    LIO lio;
};

/// pipeline/lidar_inertial_odometry.hpp:55-710 — what the reference's ROS 2 LIO node calls once per scan. The state x_ is the LiDAR
/// pose, velocity and the IMU biases in the gravity-aligned odom frame; each frame predicts it from the IMU window, hands
/// prediction and covariance to lio::LIORegistration and starts the next window from the posterior. The 15x15 arithmetic and
/// the decisions are the C library's (sp_lio_predict_state_host, sp_lio_reset_covariance_host, sp_lio_bias_observable_host,
/// sp_lio_clamp_bias_host); this class sequences them.
class LidarInertialOdometryPipeline : public odometry::PipelineCommon {
public:
    using Ptr = std::shared_ptr<LidarInertialOdometryPipeline>;
    using ConstPtr = std::shared_ptr<const LidarInertialOdometryPipeline>;

    enum class ResultType : std::int8_t {
        success = 0,
        first_frame,
        waiting_initial_alignment,
        imu_only,
        error = 100,
        old_timestamp,
        small_number_of_points,
    };

    /// :70-82
    explicit LidarInertialOdometryPipeline(const Parameters& params)
        : PipelineCommon("[LidarInertialOdometry]", "3. lio registration") {
        params_ = params;
        params_.imu.enable = true;
        adopt_imu_params(params_.imu);
        initialize();
    }

    auto get_device_queue() const { return queue_ptr_; }
    /// current / previous LiDAR pose in the gravity-aligned odom frame
    const auto& get_odom() const { return odom_; }
    const auto& get_prev_odom() const { return prev_odom_; }
    const auto& get_last_keyframe_pose() const { return submap_->get_last_keyframe_pose(); }
    const auto& get_keyframe_poses() const { return submap_->get_keyframe_poses(); }
    const PointCloudShared& get_preprocessed_point_cloud() const { return *preprocessed_pc_; }
    const PointCloudShared& get_submap_point_cloud() const { return submap_->get_submap_point_cloud(); }
    const PointCloudShared& get_last_keyframe_point_cloud() const { return submap_->get_last_keyframe_point_cloud(); }
    const auto& get_registration_result() const { return *reg_result_; }
    const imu::State& get_lio_state() const { return x_; }
    /// MI355X extension: the parameters as the constructor adjusted them (imu.enable, buffer_duration_sec)
    const Parameters& get_params() const { return params_; }
    /// MI355X extension: the posterior covariance the next IMU window starts from (LiDAR error state, 15x15)
    const Eigen::Matrix<float, 15, 15>& get_posterior_covariance() const { return P_post_; }

    /// :131-278. A first stamp of 0 reads as "no frame yet" (last_frame_time_ > 0.0, as the reference): the frame after it is not
    /// checked against it and keeps dt = -1.
    ResultType process(const PointCloudShared::Ptr scan, double timestamp) {
        error_message_.clear();
        // initial roll / pitch from stationary IMU samples, once, before the first scan becomes the reference frame (:136-144)
        if (is_first_frame_ && alignment_estimator_->enabled() && !alignment_estimator_->is_done()) {
            const imu::IMUBias current_bias{x_.gyro_bias, x_.accel_bias};
            const auto out = alignment_estimator_->try_align(timestamp, get_imu_buffer(), current_bias);
            if (out.status != imu::InitialAlignmentEstimator::Status::success) {
                error_message_ = std::string("initial_alignment: ") + out.error_message;
                return ResultType::waiting_initial_alignment;
            }
            apply_initial_alignment(out);
        }
        if (last_frame_time_ > 0.0) {  // :146-154
            const float dt = static_cast<float>(timestamp - last_frame_time_);
            if (dt > 0.0f) {
                dt_ = dt;
            } else {
                error_message_ = "old timestamp";
                return ResultType::old_timestamp;
            }
        }
        clear_current_processing_time();

        double dt_preprocessing = 0.0;
        if (!run_stage("preprocess", [&]() { time_utils::measure_execution([&]() { preprocess(scan); }, dt_preprocessing); }))
            return ResultType::error;
        {
            double dt_covariance = 0.0;
            if (!run_stage("compute_covariances", [&]() { time_utils::measure_execution([&]() { compute_covariances(); }, dt_covariance); }))
                return ResultType::error;
            add_delta_time(ProcessName::compute_covariances, dt_covariance);
        }
        {
            double dt_refine_filter = 0.0;
            if (!run_stage("refine_filter", [&]() { time_utils::measure_execution([&]() { refine_filter(); }, dt_refine_filter); }))
                return ResultType::error;
            dt_preprocessing += dt_refine_filter;
            add_delta_time(ProcessName::preprocessing, dt_preprocessing);
        }

        const bool insufficient_points = preprocessed_pc_->size() <= params_.registration.min_num_points;
        // the first frame founds the submap and cannot fall back on the IMU; rejected before the integrator advances (:198-205)
        if (is_first_frame_ && insufficient_points) {
            error_message_ = "point cloud size is too small";
            return ResultType::small_number_of_points;
        }

        integrate_imu_window(timestamp);

        if (insufficient_points) return process_imu_only(timestamp);

        if (is_first_frame_) {  // :214-244 — anchored at odom_ (post-alignment), so later frames share its frame
            if (!run_stage("build_submap (first frame)", [&]() { submap_->add_first_frame(*preprocessed_pc_, timestamp, odom_); }))
                return ResultType::error;
            is_first_frame_ = false;
            last_frame_time_ = timestamp;
            last_imu_reset_timestamp_ = timestamp;
            x_.position = odom_.translation();
            x_.rotation = sycl_points::detail::rotation_of(odom_);
            x_.velocity = Eigen::Vector3f::Zero();
            // (the biases: the parameters', the gyro's from the initial alignment when it ran)
            reset_imu_preintegration();
            return ResultType::first_frame;
        }

        {
            double dt_registration = 0.0;
            if (!run_stage("lio_registration", [&]() {
                    *reg_result_ = time_utils::measure_execution([&]() { return register_frame(); }, dt_registration);
                }))
                return ResultType::error;
            add_delta_time(ProcessName::registration, dt_registration);
        }
        last_imu_reset_timestamp_ = timestamp;

        {
            double dt_build_submap = 0.0;
            if (!run_stage("submapping", [&]() {
                    time_utils::measure_execution([&]() { submapping(*reg_result_, timestamp); }, dt_build_submap);
                }))
                return ResultType::error;
            add_delta_time(ProcessName::build_submap, dt_build_submap);
        }

        prev_odom_ = odom_;
        odom_ = reg_result_->T;
        last_frame_time_ = timestamp;
        return ResultType::success;
    }

    EIGEN_MAKE_ALIGNED_OPERATOR_NEW

private:
    static Eigen::Isometry3f state_to_pose(const imu::State& s) {  // :352-357
        Eigen::Isometry3f T = Eigen::Isometry3f::Identity();
        sycl_points::detail::set_rotation(T, s.rotation);
        for (int i = 0; i < 3; ++i) T.matrix()(i, 3) = s.position[i];
        return T;
    }
    static bool all_finite(const float* v, int n) {
        for (int i = 0; i < n; ++i)
            if (!std::isfinite(v[i])) return false;
        return true;
    }

    /// :371-393 (sp_lio_bias_observable_host) — on the window integrate_imu_window built
    bool imu_bias_observable() const {
        const auto& be = params_.lio.bias_estimation;
        std::vector<float> gyro, accel;
        gyro.reserve(3 * imu_batch_.size());
        accel.reserve(3 * imu_batch_.size());
        for (const imu::IMUMeasurement& m : imu_batch_)
            for (int k = 0; k < 3; ++k) {
                gyro.push_back(m.gyro[k]);
                accel.push_back(m.accel[k]);
            }
        int observable = 0;
        throw_on_error(sp_lio_bias_observable_host(gyro.data(), accel.data(), imu_batch_.size(), be.freeze_on_low_excitation ? 1 : 0,
                                                   be.gyro_excitation_threshold, be.accel_excitation_threshold, &observable));
        return observable != 0;
    }

    /// :402-429 (sp_lio_reset_covariance_host) — the next window starts at x_ with P_post_ plus the two floors, in the IMU's
    /// error state
    void reset_imu_preintegration() {
        const TransformMatrix T_i2l = params_.imu.T_imu_to_lidar.matrix();
        Eigen::Matrix<float, 15, 15> P_initial_imu;
        Eigen::Matrix3f R_world_imu;
        throw_on_error(sp_lio_reset_covariance_host(P_post_.data(), params_.lio.preintegration_reset.fd_velocity_sigma,
                                                    params_.lio.preintegration_reset.icp_rotation_sigma, T_i2l.data(), x_.rotation.data(),
                                                    P_initial_imu.data(), R_world_imu.data()));
        imu_preintegration_->reset(imu::IMUBias{x_.gyro_bias, x_.accel_bias}, P_initial_imu, R_world_imu);
        imu_R_world_at_reset_ = R_world_imu;
        imu_v_world_at_reset_ = x_.velocity;
    }

    /// :432-459 (sp_lio_predict_state_host)
    imu::State predict_state() const {
        const imu::IMUBias current_bias{x_.gyro_bias, x_.accel_bias};
        const TransformMatrix T_imu_rel =
            imu_preintegration_->predict_relative_transform(imu_R_world_at_reset_, imu_v_world_at_reset_, current_bias);
        const imu::PreintegrationResult c = imu_preintegration_->get_corrected(current_bias);
        const TransformMatrix T_i2l = params_.imu.T_imu_to_lidar.matrix();
        float predicted[21];
        throw_on_error(sp_lio_predict_state_host(imu::detail::PackedState(x_).v, T_i2l.data(), T_imu_rel.data(), c.Delta_v.data(),
                                                 static_cast<float>(c.dt_total), params_.imu.preintegration.gravity.data(), predicted));
        return imu::detail::unpack_state(predicted);
    }

    /// :461-470 — the IMU window [last reset, timestamp]
    void integrate_imu_window(double timestamp) {
        imu_batch_.clear();
        {
            std::lock_guard<std::mutex> lock(imu_mutex_);
            imu_batch_.reserve(imu_buffer_.size());
            imu::build_measurement_window(imu_buffer_, last_imu_reset_timestamp_, timestamp, imu_batch_);
        }
        imu_preintegration_->integrate_batch(imu_batch_);
    }

    /// :472-509 — no LiDAR update for this frame: the IMU prediction is the posterior
    ResultType process_imu_only(double timestamp) {
        const imu::State predicted_state = predict_state();
        const Eigen::Matrix<float, 15, 15> predicted_covariance = algorithms::lio::transform_covariance_imu_to_lidar(
            imu_preintegration_->get_raw().covariance, params_.imu.T_imu_to_lidar, predicted_state.rotation);
        if (!all_finite(predicted_state.position.data(), 3) || !all_finite(predicted_state.rotation.data(), 9) ||
            !all_finite(predicted_state.velocity.data(), 3) || !all_finite(predicted_covariance.data(), 225)) {
            error_message_ = "imu-only propagation produced non-finite state or covariance";
            return ResultType::error;
        }
        prev_odom_ = odom_;
        x_ = predicted_state;
        P_post_ = predicted_covariance;
        odom_ = state_to_pose(x_);

        // the previous ICP result must not stay visible as the latest one
        reg_result_->T = odom_;
        reg_result_->converged = true;
        reg_result_->iterations = 0;
        reg_result_->H.setZero();
        reg_result_->b.setZero();
        reg_result_->error = 0.0f;
        reg_result_->H_raw.setZero();
        reg_result_->b_raw.setZero();
        reg_result_->error_raw = 0.0f;
        reg_result_->inlier = 0;

        last_frame_time_ = timestamp;
        last_imu_reset_timestamp_ = timestamp;
        reset_imu_preintegration();

        error_message_ = "point cloud size is too small; propagated with IMU only";
        return ResultType::imu_only;
    }

    /// :512-537 — prediction, covariance and the sampled source go to lio::LIORegistration; its posterior starts the next window
    algorithms::registration::RegistrationResult register_frame() {
        const imu::State predicted_state = predict_state();
        const Eigen::Matrix<float, 15, 15> predicted_covariance = algorithms::lio::transform_covariance_imu_to_lidar(
            imu_preintegration_->get_raw().covariance, params_.imu.T_imu_to_lidar, predicted_state.rotation);

        const auto& sampling = params_.registration_sampling;
        PointCloudShared::ConstPtr source = preprocessed_pc_;
        if (sampling.enable && preprocessed_pc_->size() > sampling.num) {
            pc_processor_->random_sampling(*preprocessed_pc_, *registration_input_pc_, sampling.num);
            source = registration_input_pc_;
        }
        registration_source_pc_ = source;

        auto result = lio_registration_->align(*source, submap_->get_submap_point_cloud(), submap_->get_submap_kdtree(), predicted_state,
                                               predicted_covariance, P_post_, imu_bias_observable(), dt_, odom_.matrix());
        P_post_ = result.posterior_covariance;
        x_ = result.state;
        throw_on_error(sp_lio_clamp_bias_host(x_.accel_bias.data(), params_.lio.bias_estimation.max_accel_bias));
        throw_on_error(sp_lio_clamp_bias_host(x_.gyro_bias.data(), params_.lio.bias_estimation.max_gyro_bias));
        reset_imu_preintegration();
        return result.registration_result;
    }

    /// :542-601
    void initialize() {
        queue_ptr_ = std::make_shared<sycl_utils::DeviceQueue>(0);  // (params_.device is not consulted)
        preprocessed_pc_ = std::make_shared<PointCloudShared>(*queue_ptr_);
        registration_input_pc_ = std::make_shared<PointCloudShared>(*queue_ptr_);
        icp_weights_ = std::make_shared<shared_vector<float>>(*queue_ptr_);
        odom_ = params_.pose.initial;
        prev_odom_ = params_.pose.initial;
        pc_processor_ = std::make_shared<pointcloud_processing::PCProcessor>(*queue_ptr_, params_.scan, params_.covariance_estimation,
                                                                             params_.imu);
        submap_ = std::make_shared<submapping::Submap>(*queue_ptr_, params_);
        lio_registration_ =
            std::make_shared<algorithms::lio::LIORegistration>(*queue_ptr_, params_.registration.factor, params_.lio.registration);
        reg_result_ = std::make_shared<algorithms::registration::RegistrationResult>();
        {  // the first frame's reset_imu_preintegration() overwrites this with the post-alignment value before anything is integrated
            imu_preintegration_ = std::make_shared<imu::IMUPreintegration>(params_.imu.preintegration);
            const Eigen::Matrix3f R_world_imu =
                sycl_points::detail::rotation_of(params_.pose.initial) * sycl_points::detail::rotation_of(params_.imu.T_imu_to_lidar);
            imu_preintegration_->reset(params_.imu.bias, Eigen::Matrix<float, 15, 15>::Zero(), R_world_imu);
            imu_R_world_at_reset_ = R_world_imu;
            imu_v_world_at_reset_ = Eigen::Vector3f::Zero();
        }
        alignment_estimator_ = std::make_shared<imu::InitialAlignmentEstimator>(
            params_.imu.initial_alignment, params_.imu.preintegration.gravity, params_.imu.T_imu_to_lidar);
        // preprocess() deskews with the state's biases before the first frame sets the rest of the state
        x_.accel_bias = params_.imu.bias.accel_bias;
        x_.gyro_bias = params_.imu.bias.gyro_bias;
        clear_total_processing_times();
    }

    /// :619-627 — the gravity-corrected rotation with the user's yaw layered on the left; the gyro bias the alignment found. The
    /// integrator is reset by the first-frame branch.
    void apply_initial_alignment(const imu::InitialAlignmentEstimator::Output& out) {
        const float yaw_user = imu::detail::yaw_from_rotation(sycl_points::detail::rotation_of(params_.pose.initial));
        const Eigen::Matrix3f R_odom_lidar =
            Eigen::AngleAxisf(yaw_user, Eigen::Vector3f(0.0f, 0.0f, 1.0f)).toRotationMatrix() * out.R_gravity_lidar;
        x_.rotation = R_odom_lidar;
        x_.gyro_bias = out.gyro_bias;
        sycl_points::detail::set_rotation(odom_, R_odom_lidar);
        sycl_points::detail::set_rotation(prev_odom_, R_odom_lidar);
    }

    /// :632-640 — the IMU deskew gets the STATE's bias and velocity, not the parameters'
    void preprocess(const PointCloudShared::Ptr scan) {
        if (params_.imu.deskew.enable) {
            auto imu_buf = get_imu_buffer();
            const imu::IMUBias current_bias{x_.gyro_bias, x_.accel_bias};
            pc_processor_->deskew_with_imu(*scan, *scan, imu_buf, odom_, current_bias, x_.velocity);
        }
        pc_processor_->prefilter(*scan, *preprocessed_pc_);
    }

    /// :642-660
    void refine_filter() { pc_processor_->refine_filter(*preprocessed_pc_, processing_ctx_); }
    void compute_covariances() { PipelineCommon::compute_covariances(params_, *pc_processor_, *preprocessed_pc_, processing_ctx_); }

    /// :665-693 — the cloud register_frame() aligned goes into the map; robust ICP weights only when it is larger than the
    /// submap's sample
    bool submapping(const algorithms::registration::RegistrationResult& reg_result, double timestamp) {
        PointCloudShared::ConstPtr reg_pc_ptr = registration_source_pc_ != nullptr ? registration_source_pc_ : registration_input_pc_;
        bool computed_icp_weights = false;
        if (reg_pc_ptr->size() > params_.submap.point_random_sampling_num) {
            const auto& robust = params_.lio.registration.robust;
            const float robust_scale = robust.auto_scale ? robust.min_scale : params_.registration.factor.robust.default_scale;
            lio_registration_->registration_backend()->compute_icp_robust_weights(
                *reg_pc_ptr, submap_->get_submap_point_cloud(), submap_->get_submap_kdtree(), reg_result.T.matrix(), robust_scale,
                *icp_weights_);
            computed_icp_weights = true;
        }
        const float inlier_ratio =
            reg_pc_ptr->size() > 0 ? static_cast<float>(reg_result.inlier) / static_cast<float>(reg_pc_ptr->size()) : 0.0f;
        if (computed_icp_weights) return submap_->add_frame(*reg_pc_ptr, reg_result, inlier_ratio, timestamp, icp_weights_);
        return submap_->add_frame(*reg_pc_ptr, reg_result, inlier_ratio, timestamp);
    }

    sycl_utils::DeviceQueue::Ptr queue_ptr_ = nullptr;
    PointCloudShared::Ptr preprocessed_pc_ = nullptr;         // sensor frame
    PointCloudShared::Ptr registration_input_pc_ = nullptr;   // the random sample register_frame() draws
    PointCloudShared::ConstPtr registration_source_pc_ = nullptr;  // what register_frame() aligned: the sample, or preprocessed_pc_
    bool is_first_frame_ = true;
    imu::InitialAlignmentEstimator::Ptr alignment_estimator_ = nullptr;
    pointcloud_processing::ProcessingContext processing_ctx_;
    shared_vector_ptr<float> icp_weights_ = nullptr;
    pointcloud_processing::PCProcessor::Ptr pc_processor_ = nullptr;
    algorithms::lio::LIORegistration::Ptr lio_registration_ = nullptr;
    algorithms::registration::RegistrationResult::Ptr reg_result_ = nullptr;
    Eigen::Isometry3f prev_odom_;  // T_odom_to_lidar; odom_ == state_to_pose(x_) after each frame
    Eigen::Isometry3f odom_;
    submapping::Submap::Ptr submap_ = nullptr;
    double last_frame_time_ = -1.0;           // [s]
    double last_imu_reset_timestamp_ = -1.0;  // LiDAR stamp of the last preintegration reset
    float dt_ = -1.0f;                        // [s]
    Parameters params_;
    imu::State x_;
    Eigen::Matrix<float, 15, 15> P_post_ = Eigen::Matrix<float, 15, 15>::Zero();  // LiDAR error state
    imu::IMUPreintegration::Ptr imu_preintegration_ = nullptr;
    // the linearisation point of predict_relative_transform(): frozen at the reset, whatever happens to x_ afterwards
    Eigen::Matrix3f imu_R_world_at_reset_ = Eigen::Matrix3f::Identity();
    Eigen::Vector3f imu_v_world_at_reset_ = Eigen::Vector3f::Zero();
    std::vector<imu::IMUMeasurement> imu_batch_;
};

}  // namespace lidar_inertial_odometry
}  // namespace pipeline
}  // namespace sycl_points
