// Host-only C++ checks of the odometry pipeline's facade, included through the reference's paths: no device is touched, so the
// program runs in the CPU suite (tests/test_lidar_odometry_cpu.py builds it with tests/cpp/Makefile's flags).
//   InitialAlignmentEstimator::try_align waiting, succeeding, and forcing after max_wait_sec (imu_initial_alignment.hpp:273-337)
//   IMUVelocityCorrector: both formulas on a hand-computed case, the fallback before any update (imu_velocity_corrector.hpp:42-71)
//   the parameter defaults and string conversions of the reference's test_lidar_odometry_imu.cpp:90-106, the defaults the issue
//   names, what make_registration_pipeline_params() copies, MotionPredictor through the reference's types (:108-127)
// Exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <deque>

#include "sycl_points/algorithms/imu/imu_initial_alignment.hpp"
#include "sycl_points/algorithms/imu/imu_velocity_corrector.hpp"
#include "sycl_points/pipeline/lidar_odometry_params.hpp"
#include "sycl_points/pipeline/motion_predictor.hpp"
#include "sycl_points/utils/time_utils.hpp"

using namespace sycl_points;
namespace lo = sycl_points::pipeline::lidar_odometry;
namespace od = sycl_points::pipeline::odometry;
namespace reg = sycl_points::algorithms::registration;
using V3 = Eigen::Vector3f;
using M3 = Eigen::Matrix3f;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); } while (0)

static bool near(float a, float b, float tol) { return std::fabs(a - b) <= tol; }

// n samples at `rate` Hz ending at t_end, the specific force of a device rolled by `roll` (about x), gyro = bias + noise * (-1)^i
static std::deque<imu::IMUMeasurement> buffer(double t_end, double span, double rate, float roll, float gyro_noise) {
    std::deque<imu::IMUMeasurement> buf;
    const int n = (int)std::lround(span * rate);
    for (int i = 0; i <= n; ++i) {
        imu::IMUMeasurement m;
        m.timestamp = t_end - span + i / rate;
        const float s = (i & 1) ? 1.0f : -1.0f;
        m.gyro = V3(0.001f + s * gyro_noise, -0.002f, 0.0005f);
        m.accel = V3(0.0f, 9.80665f * std::sin(roll), 9.80665f * std::cos(roll));
        buf.push_back(m);
    }
    return buf;
}

static void try_align_waits_succeeds_forces() {
    imu::InitialAlignmentParams p;  // required 1 s, max_wait 5 s
    const V3 g(0.0f, 0.0f, -9.80665f);
    Eigen::Isometry3f T_i2l = Eigen::Isometry3f::Identity();
    {  // too short a buffer: waiting with the reference's text; then enough: success, done, and success again without work
        imu::InitialAlignmentEstimator est(p, g, T_i2l);
        CHECK(est.enabled() && !est.is_done());
        auto out = est.try_align(10.0, buffer(10.0, 0.5, 100.0, 0.1f, 0.0f), imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::waiting);
        CHECK(out.error_message == "IMU buffer spans less than required_duration_sec");
        CHECK(!est.is_done());
        out = est.try_align(10.6, buffer(10.6, 1.1, 100.0, 0.1f, 0.0f), imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::success && est.is_done());
        CHECK(near(out.roll_rad, 0.1f, 1e-5f) && near(out.pitch_rad, 0.0f, 1e-5f) && near(out.accel_norm, 9.80665f, 1e-4f));
        CHECK(near(out.gyro_bias[0], 0.001f, 1e-7f) && near(out.gyro_bias[1], -0.002f, 1e-7f) && near(out.gyro_bias[2], 0.0005f, 1e-7f));
        CHECK(near(out.R_gravity_lidar(2, 1), std::sin(0.1f), 1e-5f) && near(out.R_gravity_lidar(2, 2), std::cos(0.1f), 1e-5f));
        CHECK(near(imu::detail::yaw_from_rotation(out.R_gravity_lidar), 0.0f, 1e-6f));
        out = est.try_align(10.7, {}, imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::success);
    }
    {  // a shaking device: waiting until max_wait_sec has passed since the first try, then forced
        imu::InitialAlignmentEstimator est(p, g, T_i2l);
        auto out = est.try_align(20.0, buffer(20.0, 1.1, 100.0, 0.1f, 0.05f), imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::waiting);
        CHECK(out.error_message == "gyro_std exceeds threshold (robot not stationary?)");
        out = est.try_align(24.9, buffer(24.9, 1.1, 100.0, 0.1f, 0.05f), imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::waiting && !est.is_done());
        out = est.try_align(25.0, buffer(25.0, 1.1, 100.0, 0.1f, 0.05f), imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::success && est.is_done());
        CHECK(near(out.roll_rad, 0.1f, 1e-5f));
    }
    {  // max_wait_sec <= 0: never forced; a forced attempt that still cannot succeed keeps waiting
        imu::InitialAlignmentParams q = p;
        q.max_wait_sec = 0.0f;
        imu::InitialAlignmentEstimator est(q, g, T_i2l);
        est.try_align(0.5, buffer(0.5, 1.1, 100.0, 0.1f, 0.05f), imu::IMUBias());
        auto out = est.try_align(100.0, buffer(100.0, 1.1, 100.0, 0.1f, 0.05f), imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::waiting);
        imu::InitialAlignmentEstimator est2(p, g, T_i2l);
        est2.try_align(1.0, {}, imu::IMUBias());
        out = est2.try_align(7.0, buffer(7.0, 0.5, 100.0, 0.1f, 0.0f), imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::waiting);
        CHECK(out.error_message == "IMU buffer spans less than required_duration_sec");
    }
    {  // the extrinsic: R_gravity_lidar = R_world_imu * R_imu_to_lidar^T
        Eigen::Isometry3f T = Eigen::Isometry3f::Identity();
        T.matrix()(0, 0) = 0.0f; T.matrix()(0, 1) = -1.0f; T.matrix()(1, 0) = 1.0f; T.matrix()(1, 1) = 0.0f;  // Rz(90 deg)
        imu::InitialAlignmentEstimator est(p, g, T);
        const auto out = est.try_align(3.0, buffer(3.0, 1.1, 100.0, 0.0f, 0.0f), imu::IMUBias());
        CHECK(out.status == imu::InitialAlignmentEstimator::Status::success);
        CHECK(near(out.R_gravity_lidar(0, 1), 1.0f, 1e-6f) && near(out.R_gravity_lidar(1, 0), -1.0f, 1e-6f) && near(out.R_gravity_lidar(2, 2), 1.0f, 1e-6f));
    }
}

static void velocity_corrector() {
    imu::IMUVelocityCorrector c;
    imu::IMUPreintegration integ;  // no samples: Delta_v = Delta_p = 0, dt_total = 0
    // the fallback before any update; with dt = 0 in the snapshot an update changes nothing
    V3 v = c.get_reset_velocity(integ, imu::IMUBias(), V3(1.0f, 2.0f, 3.0f));
    CHECK(v[0] == 1.0f && v[1] == 2.0f && v[2] == 3.0f);
    c.update(V3(1.0f, 0.0f, 0.0f), M3::Identity(), V3(0.0f, 0.0f, -9.80665f));
    v = c.get_reset_velocity(integ, imu::IMUBias(), V3(4.0f, 5.0f, 6.0f));
    CHECK(v[0] == 4.0f && v[1] == 5.0f && v[2] == 6.0f);
    // by hand: dt = 0.5, g = (0, 0, -10), R = Rz(90 deg), dp = (0.1, 0.2, 1.25), dv = (0.4, 0.8, 5), disp = (1, 2, 0.25)
    //   R dp = (-0.2, 0.1, 1.25); 0.5 g dt^2 = (0, 0, -1.25); v_reset = ((1, 2, 0.25) - (0, 0, -1.25) - (-0.2, 0.1, 1.25)) / 0.5 = (2.4, 3.8, 0.5)
    //   R dv = (-0.8, 0.4, 5);  v_k = (2.4, 3.8, 0.5) + (0, 0, -5) + (-0.8, 0.4, 5) = (1.6, 4.2, 0.5)
    M3 Rz = M3::Identity();
    Rz(0, 0) = 0.0f; Rz(0, 1) = -1.0f; Rz(1, 0) = 1.0f; Rz(1, 1) = 0.0f;
    c.set_snapshot(V3(0.4f, 0.8f, 5.0f), V3(0.1f, 0.2f, 1.25f), 0.5f);
    c.update(V3(1.0f, 2.0f, 0.25f), Rz, V3(0.0f, 0.0f, -10.0f));
    v = c.get_reset_velocity(integ, imu::IMUBias(), V3(9.0f, 9.0f, 9.0f));
    CHECK(near(v[0], 1.6f, 1e-5f) && near(v[1], 4.2f, 1e-5f) && near(v[2], 0.5f, 1e-5f));
    // the corrected velocity is used once: the next call falls back again
    v = c.get_reset_velocity(integ, imu::IMUBias(), V3(7.0f, 8.0f, 9.0f));
    CHECK(v[0] == 7.0f && v[1] == 8.0f && v[2] == 9.0f);
    // an update without a snapshot is ignored
    imu::IMUVelocityCorrector d;
    d.update(V3(1.0f, 1.0f, 1.0f), M3::Identity(), V3(0.0f, 0.0f, -10.0f));
    v = d.get_reset_velocity(integ, imu::IMUBias(), V3(0.5f, 0.0f, 0.0f));
    CHECK(v[0] == 0.5f);
}

template <class F>
static bool throws_runtime_error(F&& f) {
    try { f(); } catch (const std::runtime_error&) { return true; }
    return false;
}

static void parameter_defaults_and_strings() {
    lo::Parameters p;
    // test_lidar_odometry_imu.cpp:90-98
    CHECK(!p.imu.enable);
    CHECK(p.motion_prediction.mode == lo::MotionPredictionMode::GYRO_LIDAR_CV);
    CHECK(p.imu.T_imu_to_lidar.matrix() == Eigen::Matrix4f::Identity());
    CHECK(near(p.imu.preintegration.gravity.norm(), 9.80665f, 1e-3f));
    CHECK(p.imu.bias.gyro_bias.norm() == 0.0f && p.imu.bias.accel_bias.norm() == 0.0f);
    // :100-106
    CHECK(lo::MotionPredictionMode_from_string("lidar_cv") == lo::MotionPredictionMode::LIDAR_CV);
    CHECK(lo::MotionPredictionMode_from_string("GYRO_LIDAR_CV") == lo::MotionPredictionMode::GYRO_LIDAR_CV);
    CHECK(lo::MotionPredictionMode_from_string("imu_se3") == lo::MotionPredictionMode::IMU_SE3);
    CHECK(lo::MotionPredictionMode_to_string(lo::MotionPredictionMode::GYRO_LIDAR_CV) == "GYRO_LIDAR_CV");
    CHECK(lo::MotionPredictionMode_to_string(lo::MotionPredictionMode::LIDAR_CV) == "LIDAR_CV");
    CHECK(lo::MotionPredictionMode_to_string(lo::MotionPredictionMode::IMU_SE3) == "IMU_SE3");
    CHECK(throws_runtime_error([] { lo::MotionPredictionMode_from_string("invalid"); }));
    CHECK(od::SubmapMapType_from_string("occupancy_grid_map") == od::SubmapMapType::OCCUPANCY_GRID_MAP);
    CHECK(od::SubmapMapType_from_string("Voxel_Hash_Map") == od::SubmapMapType::VOXEL_HASH_MAP);
    CHECK(od::SubmapMapType_to_string(od::SubmapMapType::OCCUPANCY_GRID_MAP) == "OCCUPANCY_GRID_MAP");
    CHECK(od::SubmapMapType_to_string(od::SubmapMapType::VOXEL_HASH_MAP) == "VOXEL_HASH_MAP");
    CHECK(throws_runtime_error([] { od::SubmapMapType_from_string("octomap"); }));
    // the defaults the pipeline runs with (odometry_common_params.hpp:47-227)
    CHECK(p.device.vendor == "intel" && p.device.type == "gpu");
    CHECK(p.scan.downsampling.polar.enable && !p.scan.downsampling.voxel.enable && p.scan.downsampling.random.enable);
    CHECK(p.scan.downsampling.random.num == 5000 && p.scan.downsampling.polar.coord_system == "CAMERA");
    CHECK(near(p.scan.downsampling.polar.elevation_size, 3.0f * 3.14159265f / 180.0f, 1e-7f) && p.scan.downsampling.polar.distance_size == 1.0f);
    CHECK(p.scan.preprocess.box_filter.enable && p.scan.preprocess.box_filter.min == 2.0f && p.scan.preprocess.box_filter.max == 50.0f);
    CHECK(p.scan.preprocess.angle_incidence_filter.enable && near(p.scan.preprocess.angle_incidence_filter.max_angle, 1.3962634f, 1e-6f));
    CHECK(p.scan.intensity_correction.enable && p.scan.intensity_correction.scale == 1e-3f && p.scan.intensity_correction.max_intensity == 1.0f);
    CHECK(!p.scan.intensity_gaussian.enable && !p.scan.intensity_local_mean_norm.enable && !p.scan.enhanced_reflectivity.enable);
    CHECK(p.submap.map_type == od::SubmapMapType::OCCUPANCY_GRID_MAP && p.submap.voxel_size == 1.0f && p.submap.max_distance_range == 30.0f);
    CHECK(p.submap.point_random_sampling_num == 512 && p.submap.weighted_sampling_ratio == 0.8f);
    CHECK(p.submap.keyframe.inlier_ratio_threshold == 0.7f && p.submap.keyframe.distance_threshold == 2.0f &&
          p.submap.keyframe.angle_threshold_degrees == 20.0f && p.submap.keyframe.time_threshold_seconds == 1.0f);
    CHECK(p.submap.occupancy_grid_map.log_odds_hit == 0.8f && p.submap.occupancy_grid_map.log_odds_miss == -0.05f &&
          p.submap.occupancy_grid_map.log_odds_limits_min == -1.0f && p.submap.occupancy_grid_map.log_odds_limits_max == 4.0f &&
          p.submap.occupancy_grid_map.occupied_threshold == 0.5f && p.submap.occupancy_grid_map.enable_free_space_updates &&
          p.submap.occupancy_grid_map.enable_pruning && p.submap.occupancy_grid_map.stale_frame_threshold == 100U);
    CHECK(p.covariance_estimation.neighbor_num == 10 && p.covariance_estimation.m_estimation.enable &&
          p.covariance_estimation.m_estimation.type == algorithms::robust::RobustLossType::GEMAN_MCCLURE &&
          p.covariance_estimation.m_estimation.min_robust_scale == 5.0f && p.covariance_estimation.m_estimation.max_iterations == 1);
    CHECK(p.imu.buffer_duration_sec == 1.0 && !p.imu.deskew.enable && !p.imu.deskew.gyro_only);
    CHECK(p.imu.initial_alignment.enable && p.imu.initial_alignment.required_duration_sec == 1.0f && p.imu.initial_alignment.max_wait_sec == 5.0f &&
          p.imu.initial_alignment.max_gyro_std == 0.01f && p.imu.initial_alignment.max_accel_std == 0.2f &&
          p.imu.initial_alignment.max_accel_norm_error == 0.5f && p.imu.initial_alignment.estimate_gyro_bias);
    CHECK(p.registration.min_num_points == 100 && p.registration.factor.reg_type == reg::RegType::GICP);
    CHECK(p.registration_sampling.enable && p.registration_sampling.num == 1000);
    CHECK(p.pose.initial.matrix() == Eigen::Matrix4f::Identity());
    CHECK(p.motion_prediction.velocity_ema_alpha == 1.0f && !p.motion_prediction.verbose);
    CHECK(p.motion_prediction.adaptive.rotation.min_eigenvalue_low == 5.0f && p.motion_prediction.adaptive.rotation.min_eigenvalue_high == 10.0f &&
          p.motion_prediction.adaptive.rotation.factor_min == 0.2f && p.motion_prediction.adaptive.rotation.factor_max == 1.0f);
    CHECK(p.motion_prediction.adaptive.translation.min_eigenvalue_low == 1.0f && p.motion_prediction.adaptive.translation.min_eigenvalue_high == 10.0f &&
          p.motion_prediction.adaptive.translation.factor_min == 0.2f && p.motion_prediction.adaptive.translation.factor_max == 1.0f);
    CHECK(p.lo.registration.max_iterations == 20 && !p.lo.pipeline.velocity_update.enable && !p.lo.pipeline.robust.auto_scale);
}

static void make_registration_pipeline_params_copies() {
    lo::Parameters p;
    p.registration.factor.reg_type = reg::RegType::POINT_TO_PLANE;
    p.registration.factor.max_correspondence_distance = 1.25f;
    p.registration.factor.robust.type = algorithms::robust::RobustLossType::HUBER;
    p.registration.factor.robust.default_scale = 3.5f;
    p.registration.factor.rotation_constraint.enable = true;
    p.registration.factor.genz.planarity_threshold = 0.3f;
    p.lo.registration.optimization.optimization_method = reg::OptimizationMethod::POWELL_DOGLEG;
    p.lo.registration.optimization.lm.init_lambda = 0.25f;
    p.lo.registration.optimization.dogleg.eta1 = 0.125f;
    p.lo.registration.max_iterations = 7;
    p.lo.registration.criteria.translation = 2e-4f;
    p.lo.registration.criteria.rotation = 3e-4f;
    p.lo.registration.degenerate_regularization.type = reg::DegenerateRegularizationType::nl_reg;
    p.lo.registration.degenerate_regularization.base_factor = 2.0f;
    p.lo.registration.map_prior.enabled = true;
    p.lo.registration.map_prior.rot_vel_sigma = 0.5f;
    p.registration_sampling.num = 333;
    p.registration_sampling.enable = false;
    p.lo.pipeline.robust.auto_scale = true;
    p.lo.pipeline.robust.min_scale = 0.75f;
    p.lo.pipeline.velocity_update.enable = true;
    p.lo.pipeline.velocity_update.iter = 3;
    const reg::RegistrationPipelineParams r = p.make_registration_pipeline_params();
    CHECK(r.registration.reg_type == reg::RegType::POINT_TO_PLANE && r.registration.max_correspondence_distance == 1.25f);
    CHECK(r.registration.robust.type == algorithms::robust::RobustLossType::HUBER && r.registration.robust.default_scale == 3.5f);
    CHECK(r.registration.rotation_constraint.enable && r.registration.genz.planarity_threshold == 0.3f);
    CHECK(r.registration.optimization_method == reg::OptimizationMethod::POWELL_DOGLEG && r.registration.lm.init_lambda == 0.25f &&
          r.registration.dogleg.eta1 == 0.125f);
    CHECK(r.registration.max_iterations == 7 && r.registration.criteria.translation == 2e-4f && r.registration.criteria.rotation == 3e-4f);
    CHECK(r.registration.degenerate_reg.type == reg::DegenerateRegularizationType::nl_reg && r.registration.degenerate_reg.base_factor == 2.0f);
    CHECK(r.registration.map_prior.enabled && r.registration.map_prior.rot_vel_sigma == 0.5f);
    CHECK(r.random_sampling.num == 333 && !r.random_sampling.enable);
    CHECK(r.robust.auto_scale && r.robust.min_scale == 0.75f);
    CHECK(r.velocity_update.enable && r.velocity_update.iter == 3);
    // the two-argument constructor alone: the halves are copied, the rest keeps its defaults
    const reg::RegistrationParams q(p.registration.factor, p.lo.registration.optimization);
    CHECK(q.reg_type == reg::RegType::POINT_TO_PLANE && q.optimization_method == reg::OptimizationMethod::POWELL_DOGLEG &&
          q.max_iterations == 20 && q.criteria.translation == 1e-3f && !q.map_prior.enabled);
}

static void motion_predictor_known_answer() {  // test_lidar_odometry_imu.cpp:108-127 through the reference's types
    lo::MotionPredictor::Params params;
    params.mode = lo::MotionPredictionMode::GYRO_LIDAR_CV;
    lo::MotionPredictor predictor(params);
    Eigen::Isometry3f odom = Eigen::Isometry3f::Identity();
    odom.matrix()(0, 3) = 2.0f; odom.matrix()(1, 3) = -1.0f; odom.matrix()(2, 3) = 0.5f;
    const M3 delta_R_imu = Eigen::AngleAxisf(0.4f, V3(0.0f, 0.0f, 1.0f)).toRotationMatrix();
    lo::MotionPredictionCandidates candidates;
    candidates.gyro_delta_rotation_lidar = delta_R_imu;
    const auto reg_result = std::make_shared<reg::RegistrationResult>();
    const Eigen::Isometry3f fused =
        predictor.predict(V3(1.0f, 2.0f, 3.0f), Eigen::AngleAxisf(0.2f, V3(1.0f, 0.0f, 0.0f)), odom, 1.0f, reg_result, false, candidates);
    const V3 t = fused.translation();
    CHECK(near(t[0], 3.0f, 1e-5f) && near(t[1], 1.0f, 1e-5f) && near(t[2], 3.5f, 1e-5f));
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) CHECK(near(fused.rotation()(i, j), delta_R_imu(i, j), 1e-5f));
    CHECK(near(delta_R_imu(0, 0), std::cos(0.4f), 1e-6f) && near(delta_R_imu(1, 0), std::sin(0.4f), 1e-6f));
    // the adaptive predictor alone turns by the angular velocity: Rx(0.2)
    lo::AdaptiveMotionPredictor cv(params);
    const Eigen::Isometry3f pred = cv.predict(V3(1.0f, 2.0f, 3.0f), Eigen::AngleAxisf(0.2f, V3(1.0f, 0.0f, 0.0f)), odom, 1.0f, reg_result, false);
    CHECK(near(pred.rotation()(2, 1), std::sin(0.2f), 1e-5f) && near(pred.rotation()(1, 1), std::cos(0.2f), 1e-5f) && near(pred.rotation()(0, 0), 1.0f, 1e-6f));
    CHECK(cv.last_factors().first == 1.0f && cv.last_factors().second == 1.0f);
}

static void measure_execution_adds() {
    double us = 5.0;
    const int v = time_utils::measure_execution([](int a) { return a + 1; }, us, 41);
    CHECK(v == 42 && us >= 5.0);
    time_utils::measure_execution([] {}, us);
    CHECK(us >= 5.0);
}

int main() {
    RUN(try_align_waits_succeeds_forces);
    RUN(velocity_corrector);
    RUN(parameter_defaults_and_strings);
    RUN(make_registration_pipeline_params_copies);
    RUN(motion_predictor_known_answer);
    RUN(measure_execution_adds);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
