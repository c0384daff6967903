// sycl_points facade for MI355X — IMU layer.
//   algorithms/imu/imu_preintegration.hpp : imu::IMUMeasurement, interpolate_measurement, imu_measurement_range,
//                                           build_measurement_window, IMUBias, PreintegrationJacobians, PreintegrationResult,
//                                           IMUPreintegrationParams, IMUPreintegration
//   algorithms/deskew/imu_deskew.hpp      : deskew::IMUTrajectoryPose, IMUDeskewStatus, deskew_point_cloud_imu
// The integrator is the C library's host code (sp_imu_preint_*): one copy of the arithmetic, shared with the Python mirror.
// The deskew builds its trajectory on the host (sp_imu_deskew_trajectory_host, sp_imu_deskew_intervals_host) and moves the
// points with one kernel (sp_deskew_imu); data stays on the device.
#pragma once
#include <algorithm>
#include <cmath>
#include <concepts>
#include <iterator>
#include <memory>
#include <ranges>
#include <stdexcept>
#include <vector>

#include "core.hpp"

namespace sycl_points {
namespace imu {

/// imu_preintegration.hpp:17-23
struct IMUMeasurement {
    double timestamp = 0.0;                           ///< absolute time [s]
    Eigen::Vector3f gyro = Eigen::Vector3f::Zero();   ///< angular velocity [rad/s], body frame, raw
    Eigen::Vector3f accel = Eigen::Vector3f::Zero();  ///< linear acceleration [m/s^2], body frame, raw
};

/// imu_preintegration.hpp:32-42 — linear interpolation between two samples (in double, as the reference)
inline IMUMeasurement interpolate_measurement(const IMUMeasurement& before, const IMUMeasurement& after, double timestamp) {
    const double span = after.timestamp - before.timestamp;
    if (span <= 0.0) return before;
    const double alpha = std::clamp((timestamp - before.timestamp) / span, 0.0, 1.0);
    IMUMeasurement out;
    out.timestamp = timestamp;
    for (int k = 0; k < 3; ++k) {
        out.gyro[k] = static_cast<float>((1.0 - alpha) * static_cast<double>(before.gyro[k]) + alpha * static_cast<double>(after.gyro[k]));
        out.accel[k] = static_cast<float>((1.0 - alpha) * static_cast<double>(before.accel[k]) + alpha * static_cast<double>(after.accel[k]));
    }
    return out;
}

/// imu_preintegration.hpp:44-47
template <typename Range>
concept imu_measurement_range = std::ranges::range<Range> && requires(Range& r) {
    { *std::begin(r) } -> std::convertible_to<IMUMeasurement>;
};

/// imu_preintegration.hpp:55-87 — the samples of (start, end] with one interpolated at either boundary when bracketed
template <imu_measurement_range Range>
void build_measurement_window(const Range& measurements, double start_timestamp, double end_timestamp,
                              std::vector<IMUMeasurement>& window) {
    window.clear();
    if (end_timestamp <= start_timestamp) return;
    IMUMeasurement before_start;
    bool has_before_start = false;
    for (const auto& measurement : measurements) {
        if (measurement.timestamp <= start_timestamp) {
            before_start = measurement;
            has_before_start = true;
            continue;
        }
        if (measurement.timestamp > end_timestamp) {
            if (window.empty() && has_before_start) window.push_back(interpolate_measurement(before_start, measurement, start_timestamp));
            if (!window.empty() && window.back().timestamp < end_timestamp)
                window.push_back(interpolate_measurement(window.back(), measurement, end_timestamp));
            break;
        }
        if (window.empty() && has_before_start)
            window.push_back(before_start.timestamp < start_timestamp ? interpolate_measurement(before_start, measurement, start_timestamp)
                                                                      : before_start);
        window.push_back(measurement);
    }
}

/// imu_preintegration.hpp:90-95
struct IMUBias {
    Eigen::Vector3f gyro_bias = Eigen::Vector3f::Zero();   ///< [rad/s]
    Eigen::Vector3f accel_bias = Eigen::Vector3f::Zero();  ///< [m/s^2]
};

/// imu_preintegration.hpp:98-106
struct PreintegrationJacobians {
    Eigen::Matrix3f J_R_bg = Eigen::Matrix3f::Zero();
    Eigen::Matrix3f J_v_bg = Eigen::Matrix3f::Zero();
    Eigen::Matrix3f J_v_ba = Eigen::Matrix3f::Zero();
    Eigen::Matrix3f J_p_bg = Eigen::Matrix3f::Zero();
    Eigen::Matrix3f J_p_ba = Eigen::Matrix3f::Zero();
};

/// imu_preintegration.hpp:109-135; covariance order [dp, dphi, dv, dba, dbg]
struct PreintegrationResult {
    Eigen::Matrix3f Delta_R = Eigen::Matrix3f::Identity();
    Eigen::Vector3f Delta_v = Eigen::Vector3f::Zero();
    Eigen::Vector3f Delta_p = Eigen::Vector3f::Zero();
    double dt_total = 0.0;
    PreintegrationJacobians J;
    Eigen::Matrix<float, 15, 15> covariance = Eigen::Matrix<float, 15, 15>::Zero();
};

/// imu_preintegration.hpp:138-166
struct IMUPreintegrationParams {
    Eigen::Vector3f gravity = Eigen::Vector3f(0.0f, 0.0f, -9.80665f);
    float accel_scale = 1.0f;
    float gyro_noise_density = 0.0f;
    float accel_noise_density = 0.0f;
    float gyro_bias_rw_density = 0.0f;
    float accel_bias_rw_density = 0.0f;
};

namespace detail {
inline sp_imu_params to_c(const IMUPreintegrationParams& p) {
    sp_imu_params c;
    for (int k = 0; k < 3; ++k) c.gravity[k] = p.gravity[k];
    c.accel_scale = p.accel_scale;
    c.gyro_noise_density = p.gyro_noise_density;
    c.accel_noise_density = p.accel_noise_density;
    c.gyro_bias_rw_density = p.gyro_bias_rw_density;
    c.accel_bias_rw_density = p.accel_bias_rw_density;
    return c;
}
struct Bias6 {
    float v[6];
    explicit Bias6(const IMUBias& b) {
        for (int k = 0; k < 3; ++k) {
            v[k] = b.gyro_bias[k];
            v[3 + k] = b.accel_bias[k];
        }
    }
};
}  // namespace detail

/// imu_preintegration.hpp:180-529 — on-manifold preintegration with the midpoint rule, over the C library's handle.
/// Movable, not copyable (the reference's is copyable; nothing in it copies one).
class IMUPreintegration {
public:
    using Ptr = std::shared_ptr<IMUPreintegration>;

    explicit IMUPreintegration(const IMUPreintegrationParams& params = IMUPreintegrationParams()) : params_(params) {
        const sp_imu_params c = detail::to_c(params);
        throw_on_error(sp_imu_preint_create(&c, &handle_));
    }
    ~IMUPreintegration() { sp_imu_preint_destroy(handle_); }
    IMUPreintegration(const IMUPreintegration&) = delete;
    IMUPreintegration& operator=(const IMUPreintegration&) = delete;
    IMUPreintegration(IMUPreintegration&& o) noexcept : params_(o.params_), handle_(o.handle_) { o.handle_ = nullptr; }

    void reset(const IMUBias& bias = IMUBias(),
               const Eigen::Matrix<float, 15, 15>& initial_covariance = Eigen::Matrix<float, 15, 15>::Zero(),
               const Eigen::Matrix3f& R_world_body = Eigen::Matrix3f::Identity()) {
        throw_on_error(sp_imu_preint_reset(handle_, detail::Bias6(bias).v, initial_covariance.data(), R_world_body.data()));
    }

    void integrate(const IMUMeasurement& meas) {
        throw_on_error(sp_imu_preint_integrate(handle_, meas.timestamp, meas.gyro.data(), meas.accel.data()));
    }

    template <std::ranges::range Range>
        requires std::same_as<std::ranges::range_value_t<Range>, IMUMeasurement>
    void integrate_batch(const Range& measurements) {
        for (const auto& m : measurements) integrate(m);
    }

    PreintegrationResult get_corrected(const IMUBias& new_bias) const { return fetch(detail::Bias6(new_bias).v); }
    const PreintegrationResult& get_raw() const {
        raw_ = fetch(nullptr);
        return raw_;
    }

    TransformMatrix predict_transform(const TransformMatrix& T_world_body_i, const Eigen::Vector3f& v_world_i,
                                      const IMUBias& current_bias) const {
        TransformMatrix T;
        throw_on_error(sp_imu_preint_predict_transform(handle_, T_world_body_i.data(), v_world_i.data(), detail::Bias6(current_bias).v, T.data()));
        return T;
    }
    TransformMatrix predict_relative_transform(const Eigen::Matrix3f& R_world_body_i, const Eigen::Vector3f& v_world_i,
                                               const IMUBias& current_bias) const {
        TransformMatrix T;
        throw_on_error(sp_imu_preint_predict_relative(handle_, R_world_body_i.data(), v_world_i.data(), detail::Bias6(current_bias).v, T.data()));
        return T;
    }

    double get_dt_total() const { return fetch(nullptr).dt_total; }
    bool has_measurements() const { return sp_imu_preint_num_measurements(handle_) > 0; }
    const IMUPreintegrationParams& get_params() const { return params_; }

private:
    PreintegrationResult fetch(const float* bias6) const {
        sp_imu_state s;
        throw_on_error(sp_imu_preint_get(handle_, bias6, &s));
        PreintegrationResult r;
        auto m3 = [](const float* a) { Eigen::Matrix3f m; for (int k = 0; k < 9; ++k) m.data()[k] = a[k]; return m; };
        r.Delta_R = m3(s.Delta_R);
        for (int k = 0; k < 3; ++k) {
            r.Delta_v[k] = s.Delta_v[k];
            r.Delta_p[k] = s.Delta_p[k];
        }
        r.dt_total = s.dt_total;
        r.J.J_R_bg = m3(s.J_R_bg);
        r.J.J_v_bg = m3(s.J_v_bg);
        r.J.J_v_ba = m3(s.J_v_ba);
        r.J.J_p_bg = m3(s.J_p_bg);
        r.J.J_p_ba = m3(s.J_p_ba);
        for (int k = 0; k < 225; ++k) r.covariance.data()[k] = s.covariance[k];
        return r;
    }

    IMUPreintegrationParams params_;
    void* handle_ = nullptr;
    mutable PreintegrationResult raw_;
};

}  // namespace imu

namespace algorithms {
namespace deskew {

/// imu_deskew.hpp:23-29 — the LiDAR frame at a time of the scan relative to the frame at scan start
struct IMUTrajectoryPose {
    Eigen::Vector4f q;  ///< unit quaternion x, y, z, w
    Eigen::Vector3f t;  ///< translation in the scan-start LiDAR frame [m]
    float timestamp;    ///< time from scan start [s]
};
static_assert(sizeof(IMUTrajectoryPose) == 32, "IMUTrajectoryPose size mismatch");

/// imu_deskew.hpp:32-38 (the values are the C ABI's SP_IMU_DESKEW_*)
enum class IMUDeskewStatus {
    success = SP_IMU_DESKEW_SUCCESS,
    insufficient_imu_coverage = SP_IMU_DESKEW_INSUFFICIENT_IMU_COVERAGE,
    no_timestamps = SP_IMU_DESKEW_NO_TIMESTAMPS,
    invalid_scan_duration = SP_IMU_DESKEW_INVALID_SCAN_DURATION,
    empty_cloud = SP_IMU_DESKEW_EMPTY_CLOUD,
};

/// imu_deskew.hpp:122-417 — every point is brought into the sensor frame at scan start along the trajectory the buffered IMU
/// samples give (gravity compensated with R_world_body_i as predict_relative_transform does; gyro_only: rotation alone). The
/// trajectory is integrated on the host, its interval table goes up through the queue's staging, one kernel moves points,
/// normals and covariances. In place (`&input_cloud == &output_cloud`) is allowed and — unlike the reference, which zeroes its
/// outputs before it reads its inputs — returns the rotated normals and covariances. false with *status set: an empty cloud, a
/// cloud without time stamps, a scan duration <= 0, IMU samples that do not cover the scan.
template <imu::imu_measurement_range Range>
inline bool deskew_point_cloud_imu(const PointCloudShared& input_cloud, PointCloudShared& output_cloud, const Range& imu_buffer,
                                   double scan_start_time_sec, const Eigen::Isometry3f& T_imu_to_lidar, const imu::IMUBias& bias,
                                   const imu::IMUPreintegrationParams& preintegration_params, const Eigen::Matrix3f& R_world_body_i,
                                   const Eigen::Vector3f& v_world_body_i, IMUDeskewStatus* status = nullptr, bool gyro_only = false) {
    auto set_status = [&](IMUDeskewStatus s) {
        if (status) *status = s;
    };
    if (!input_cloud.queue.ptr || !output_cloud.queue.ptr)
        throw std::runtime_error("[deskew_point_cloud_imu] SYCL queue is not initialized");
    const size_t N = input_cloud.size();
    if (N == 0) {
        set_status(IMUDeskewStatus::empty_cloud);
        return false;
    }
    if (!input_cloud.has_timestamps()) {
        set_status(IMUDeskewStatus::no_timestamps);
        return false;
    }
    const double scan_duration_sec = (input_cloud.end_time_ms - input_cloud.start_time_ms) * 1e-3;
    // steps 1-3 on the host
    std::vector<double> stamps;
    std::vector<float> gyro_accel;
    for (const imu::IMUMeasurement& m : imu_buffer) {
        stamps.push_back(m.timestamp);
        for (int k = 0; k < 3; ++k) gyro_accel.push_back(m.gyro[k]);
        for (int k = 0; k < 3; ++k) gyro_accel.push_back(m.accel[k]);
    }
    std::vector<IMUTrajectoryPose> traj(stamps.size() + 1);
    const sp_imu_params params = imu::detail::to_c(preintegration_params);
    size_t n_traj = 0;
    int code = 0;
    throw_on_error(sp_imu_deskew_trajectory_host(stamps.data(), gyro_accel.data(), stamps.size(), scan_start_time_sec, scan_duration_sec,
                                                 T_imu_to_lidar.matrix().data(), imu::detail::Bias6(bias).v, &params,
                                                 R_world_body_i.data(), v_world_body_i.data(), gyro_only ? 1 : 0,
                                                 reinterpret_cast<float*>(traj.data()), traj.size(), &n_traj, &code));
    if (code != SP_IMU_DESKEW_SUCCESS) {
        set_status(static_cast<IMUDeskewStatus>(code));
        return false;
    }
    // step 4: one row per interval, uploaded on the queue's stream (no device-wide wait)
    std::vector<float> rows(16 * (n_traj - 1));
    throw_on_error(sp_imu_deskew_intervals_host(reinterpret_cast<const float*>(traj.data()), n_traj, rows.data()));
    shared_vector<float> table(input_cloud.queue);
    table.assign(rows.data(), rows.size());
    // step 5 (:297-325): the output mirrors the input's timing and the attributes the deskew does not touch; step 6: the kernel
    const sycl_points::detail::DeskewBuffers b = sycl_points::detail::prepare_deskew_output(input_cloud, output_cloud);
    throw_on_error(sp_deskew_imu(b.points_in, b.covs_in, b.normals_in, input_cloud.timestamp_offsets->device_data(), N, table.device_data(),
                                 n_traj - 1, b.points_out, b.covs_out, b.normals_out, input_cloud.queue.stream()));
    sycl_utils::events(input_cloud.queue.stream()).wait_and_throw();  // :413
    set_status(IMUDeskewStatus::success);
    return true;
}

}  // namespace deskew
}  // namespace algorithms
}  // namespace sycl_points
