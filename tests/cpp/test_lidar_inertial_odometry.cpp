// C++ tests of pipeline::lidar_inertial_odometry::LidarInertialOdometryPipeline, included through the reference's paths only. Built
// and run by tests/test_gpu_lidar_inertial_odometry.py on a GPU box: test_lidar_inertial_odometry <golden dir>; exit code 0 = all
// checks passed.
//   1. pipeline_is_the_chain   target.ply at 1.0 and source.ply at 1.1 with a resting IMU against the same calls made by hand on
//                              fresh objects: pose, state, posterior covariance, preprocessed row counts (bit for bit when two hand
//                              runs agree bit for bit, else within four times their largest entry difference)
//   2. drive_from_rest         five frames from rest at 4 m/s^2 and 10 deg/s, both submap types: relative motion, final velocity
//   3. imu_only                a 50-point frame in that drive: IMU propagation against a hand-integrated window, the recovery
//                              on the next full frame; a 50-point FIRST frame is rejected and leaves nothing behind
//   4. result_codes            old_timestamp, error with "preprocess: ...", the four timing keys
//   5. bias_rules              freeze_on_low_excitation at rest keeps the biases; max_gyro_bias clamps
//   6. invalid_prior           all noise densities 0: the regularisation branch of the alignment
//   7. initial_alignment       the gate, the aligned first frame against the estimator called by hand, the adjusted parameters
//   8. deskew_uses_state       the IMU deskew of the caller's scan, in place, with the state's bias and velocity
// Shared settings: T_imu_to_lidar = identity, IMU at 200 Hz covering every frame stamp, first frame stamp 1.0, the noise densities
// of the reference's config/lidar_inertial_odometry.yaml (gyro 1e-2, accel 1e-3, and its bias random walks 1e-5 / 1e-4: with the
// struct's zeros the predicted covariance is singular, the prior invalid and only the regularisation branch runs - case 6), the
// initial alignment off except in case 7. Every figure is printed before it is checked.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sycl_points/algorithms/deskew/imu_deskew.hpp"
#include "sycl_points/algorithms/imu/imu_initial_alignment.hpp"
#include "sycl_points/algorithms/imu/imu_preintegration.hpp"
#include "sycl_points/algorithms/lio/lio_registration.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"
#include "sycl_points/pipeline/lidar_inertial_odometry.hpp"
#include "sycl_points/pipeline/pointcloud_processing.hpp"
#include "sycl_points/pipeline/submapping.hpp"

using namespace sycl_points;
namespace alg = sycl_points::algorithms;
namespace lio = sycl_points::pipeline::lidar_inertial_odometry;
namespace od = sycl_points::pipeline::odometry;
namespace pp = sycl_points::pipeline::pointcloud_processing;
using Pipeline = lio::LidarInertialOdometryPipeline;
using Result = Pipeline::ResultType;
using V3 = Eigen::Vector3f;
using M3 = Eigen::Matrix3f;
using M4 = Eigen::Matrix4f;
using M15 = Eigen::Matrix<float, 15, 15>;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); std::fflush(stdout); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); std::fflush(stdout); } while (0)

static constexpr float kPi = 3.14159265358979323846f;
static constexpr float kG = 9.80665f;
static constexpr float kTransBound = 0.05f, kRotBound = 0.01f;  // the project's drive bound (tests/cpp/test_lidar_odometry.cpp)
static constexpr double kImuPeriod = 0.005;                     // 200 Hz
static constexpr double kFramePeriod = 0.1;
static PointCloudCPU g_target, g_source;

// ------------------------------------------------------------------------------------------------ helpers
static M4 rigid(float yaw, float x, float y = 0.0f, float z = 0.0f) {
    M4 T = M4::Identity();
    T(0, 0) = std::cos(yaw); T(0, 1) = -std::sin(yaw); T(1, 0) = std::sin(yaw); T(1, 1) = std::cos(yaw);
    T(0, 3) = x; T(1, 3) = y; T(2, 3) = z;
    return T;
}
static Eigen::Isometry3f iso(const M4& M) {
    Eigen::Isometry3f T = Eigen::Isometry3f::Identity();
    T.matrix() = M;
    return T;
}
static M4 relative(const M4& A, const M4& B) { return (iso(A).inverse() * iso(B)).matrix(); }
template <class A, class B>
static float max_diff(const A& a, const B& b, int n) {
    float d = 0.0f;
    for (int k = 0; k < n; ++k) d = std::max(d, std::fabs(a[k] - b[k]));
    return d;
}
static float max_entry_diff(const M4& A, const M4& B) { return max_diff(A.data(), B.data(), 16); }
static void pose_error(const M4& T, const M4& ref, float* trans, float* rot) {
    const float dx = T(0, 3) - ref(0, 3), dy = T(1, 3) - ref(1, 3), dz = T(2, 3) - ref(2, 3);
    *trans = std::sqrt(dx * dx + dy * dy + dz * dz);
    *rot = 0.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) *rot = std::max(*rot, std::fabs(T(i, j) - ref(i, j)));
}
static bool all_finite(const float* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}
/// the cloud as a sensor at pose T (in the cloud's frame) sees it: p' = T^-1 p, in double
static PointCloudCPU seen_from(const PointCloudCPU& cloud, const M4& T) {
    PointCloudCPU out;
    out.points->resize(cloud.size());
    *out.intensities = *cloud.intensities;
    for (size_t i = 0; i < cloud.size(); ++i) {
        const PointType& p = (*cloud.points)[i];
        const double d[3] = {double(p[0]) - T(0, 3), double(p[1]) - T(1, 3), double(p[2]) - T(2, 3)};
        PointType q(0.0f, 0.0f, 0.0f, 1.0f);
        for (int r = 0; r < 3; ++r) q[r] = float(double(T(0, r)) * d[0] + double(T(1, r)) * d[1] + double(T(2, r)) * d[2]);
        (*out.points)[i] = q;
    }
    return out;
}
/// n points of the cloud, spread over it, between 3 m and 40 m (inside the box filter)
static PointCloudCPU subset(const PointCloudCPU& cloud, size_t n) {
    PointCloudCPU out;
    for (size_t i = 0; i < cloud.size() && out.size() < n; i += 97) {
        const PointType& p = (*cloud.points)[i];
        const float range = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        if (range > 3.0f && range < 40.0f) {
            out.points->push_back(p);
            if (cloud.has_intensity()) out.intensities->push_back((*cloud.intensities)[i]);
        }
    }
    return out;
}
static PointCloudShared::Ptr upload(const Pipeline& p, const PointCloudCPU& cpu) {
    return std::make_shared<PointCloudShared>(*p.get_device_queue(), cpu);
}
static void pack(const imu::State& x, float* v21) { std::memcpy(v21, imu::detail::PackedState(x).v, 21 * sizeof(float)); }
static bool same_state(const imu::State& a, const imu::State& b) {
    float va[21], vb[21];
    pack(a, va);
    pack(b, vb);
    return std::memcmp(va, vb, sizeof(va)) == 0;
}
static float state_diff(const imu::State& a, const imu::State& b) {
    float va[21], vb[21];
    pack(a, va);
    pack(b, vb);
    return max_diff(va, vb, 21);
}
static M4 pose_of(const imu::State& x) {
    M4 T = M4::Identity();
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T(i, j) = x.rotation(i, j);
        T(i, 3) = x.position[i];
    }
    return T;
}
static void print_pose(const char* label, const M4& T) {
    std::printf("  %s\n", label);
    for (int r = 0; r < 4; ++r) std::printf("    % .9g % .9g % .9g % .9g\n", T(r, 0), T(r, 1), T(r, 2), T(r, 3));
}
static void print_state(const char* label, const imu::State& x) {
    std::printf("  %s: p (% .6g % .6g % .6g) v (% .6g % .6g % .6g) b_a (% .3g % .3g % .3g) b_g (% .3g % .3g % .3g)\n", label, x.position[0],
                x.position[1], x.position[2], x.velocity[0], x.velocity[1], x.velocity[2], x.accel_bias[0], x.accel_bias[1],
                x.accel_bias[2], x.gyro_bias[0], x.gyro_bias[1], x.gyro_bias[2]);
}

static lio::Parameters shared_params() {
    lio::Parameters p;
    p.imu.initial_alignment.enable = false;
    p.imu.preintegration.gyro_noise_density = 1e-2f;
    p.imu.preintegration.accel_noise_density = 1e-3f;
    p.imu.preintegration.gyro_bias_rw_density = 1e-5f;
    p.imu.preintegration.accel_bias_rw_density = 1e-4f;
    return p;
}

// ------------------------------------------------------------------------------------------------ the IMU
static imu::IMUMeasurement sample(double t, const V3& gyro, const V3& accel) {
    imu::IMUMeasurement m;
    m.timestamp = t;
    m.gyro = gyro;
    m.accel = accel;
    return m;
}
static double tick_time(int tick) { return tick * kImuPeriod; }
static double frame_time(int k) { return tick_time(200 + 20 * k); }  // 1.0, 1.1, ...
static imu::IMUMeasurement resting(int tick) { return sample(tick_time(tick), V3(0.0f, 0.0f, 0.0f), V3(0.0f, 0.0f, kG)); }

// the drive: from rest at t = 1.0, acceleration (4, 0, 0) m/s^2 in the world, yaw rate 10 deg/s
static constexpr double kAccel = 4.0, kYawRate = 10.0 * 3.14159265358979323846 / 180.0;
static M4 drive_pose(double t) {
    const double s = t - 1.0;
    return rigid(float(kYawRate * s), float(0.5 * kAccel * s * s));
}
/// at rest before t = 1.0; from then on the specific force R(t)^T (a - g) and the gyro (0, 0, w)
static imu::IMUMeasurement driving(int tick) {
    if (tick < 200) return resting(tick);
    const double yaw = kYawRate * (tick_time(tick) - 1.0);
    return sample(tick_time(tick), V3(0.0f, 0.0f, float(kYawRate)),
                  V3(float(std::cos(yaw) * kAccel), float(-std::sin(yaw) * kAccel), kG));
}
template <class F>
static void feed(Pipeline& p, int tick_from, int tick_to, F&& measurement) {
    for (int tick = tick_from; tick <= tick_to; ++tick) p.add_imu_measurement(measurement(tick));
}

/// the drive's samples a stream has delivered when frame k arrives: from 0.9 s up to two samples past the frame's stamp
static void feed_until_frame(Pipeline& p, int k) {
    feed(p, k == 0 ? 180 : 200 + 20 * (k - 1) + 3, 200 + 20 * k + 2, driving);
}

// ------------------------------------------------------------------------------------------------ the pipeline's IMU side by hand
/// reset_imu_preintegration with the C library's function
static void hand_reset(const lio::Parameters& P, imu::IMUPreintegration& integ, const imu::State& x, const M15& P_post, M3* R_at_reset,
                       V3* v_at_reset) {
    M15 P_initial_imu;
    M3 R_world_imu;
    const M4 T_i2l = P.imu.T_imu_to_lidar.matrix();
    throw_on_error(sp_lio_reset_covariance_host(P_post.data(), P.lio.preintegration_reset.fd_velocity_sigma,
                                                P.lio.preintegration_reset.icp_rotation_sigma, T_i2l.data(), x.rotation.data(),
                                                P_initial_imu.data(), R_world_imu.data()));
    integ.reset(imu::IMUBias{x.gyro_bias, x.accel_bias}, P_initial_imu, R_world_imu);
    *R_at_reset = R_world_imu;
    *v_at_reset = x.velocity;
}
/// predict_state with the C library's function
static imu::State hand_predict(const lio::Parameters& P, const imu::IMUPreintegration& integ, const imu::State& x, const M3& R_at_reset,
                               const V3& v_at_reset) {
    const imu::IMUBias bias{x.gyro_bias, x.accel_bias};
    const M4 T_rel = integ.predict_relative_transform(R_at_reset, v_at_reset, bias);
    const imu::PreintegrationResult c = integ.get_corrected(bias);
    const M4 T_i2l = P.imu.T_imu_to_lidar.matrix();
    float out[21];
    throw_on_error(sp_lio_predict_state_host(imu::detail::PackedState(x).v, T_i2l.data(), T_rel.data(), c.Delta_v.data(), float(c.dt_total),
                                             P.imu.preintegration.gravity.data(), out));
    return imu::detail::unpack_state(out);
}
static bool hand_observable(const lio::Parameters& P, const std::vector<imu::IMUMeasurement>& window) {
    std::vector<float> gyro, accel;
    for (const auto& m : window)
        for (int k = 0; k < 3; ++k) {
            gyro.push_back(m.gyro[k]);
            accel.push_back(m.accel[k]);
        }
    int flag = 0;
    const auto& be = P.lio.bias_estimation;
    throw_on_error(sp_lio_bias_observable_host(gyro.data(), accel.data(), window.size(), be.freeze_on_low_excitation ? 1 : 0,
                                               be.gyro_excitation_threshold, be.accel_excitation_threshold, &flag));
    return flag != 0;
}

// ------------------------------------------------------------------------------------------------ 1. the chain, by hand
struct HandResult {
    M4 pose;
    imu::State state;
    M15 P_post;
    size_t rows_first, rows_second;
    uint32_t inlier;
    size_t iterations;
    bool prior_valid;
    imu::State first_state;
};
/// What process() does for two frames with the shared settings and a resting IMU, call by call on fresh objects: ONE PCProcessor for
/// both frames (the pipeline's: its samplers draw from one generator), a Submap, an IMUPreintegration reset and read through the
/// C library's functions, LIORegistration::align, clamp, reset.
static HandResult hand_chain() {
    const lio::Parameters P = [] { lio::Parameters p = shared_params(); p.imu.enable = true; return p; }();
    const double t0 = frame_time(0), t1 = frame_time(1);
    sycl_utils::DeviceQueue q(0);
    pp::PCProcessor proc(q, P.scan, P.covariance_estimation, P.imu);
    pipeline::submapping::Submap submap(q, P);
    alg::lio::LIORegistration registration(q, P.registration.factor, P.lio.registration);
    std::deque<imu::IMUMeasurement> buffer;
    for (int tick = 180; tick <= 240; ++tick) buffer.push_back(resting(tick));

    imu::State x;  // initialize(): the biases of the parameters
    x.accel_bias = P.imu.bias.accel_bias;
    x.gyro_bias = P.imu.bias.gyro_bias;
    Eigen::Isometry3f odom = P.pose.initial;
    M15 P_post = M15::Zero();
    imu::IMUPreintegration integ(P.imu.preintegration);
    M3 R_at_reset = M3::Identity();
    V3 v_at_reset = V3::Zero();
    integ.reset(P.imu.bias, M15::Zero(), M3::Identity());
    std::vector<imu::IMUMeasurement> window;
    double last_reset = -1.0;

    auto front_end = [&](const PointCloudCPU& cpu) {
        PointCloudShared scan(q, cpu);
        auto pc = std::make_shared<PointCloudShared>(q);
        if (P.imu.deskew.enable) proc.deskew_with_imu(scan, scan, buffer, odom, imu::IMUBias{x.gyro_bias, x.accel_bias}, x.velocity);
        proc.prefilter(scan, *pc);
        pp::ProcessingContext ctx = proc.prepare_context(*pc);  // (GICP: the covariances are needed)
        proc.compute_covariances(*pc, ctx);
        proc.refine_filter(*pc, ctx);
        return pc;
    };
    HandResult out;
    // frame 1
    const auto first = front_end(g_target);
    imu::build_measurement_window(buffer, last_reset, t0, window);
    integ.integrate_batch(window);
    submap.add_first_frame(*first, t0, odom);
    last_reset = t0;
    x.position = odom.translation();
    x.rotation = odom.rotation();
    x.velocity = V3::Zero();
    hand_reset(P, integ, x, P_post, &R_at_reset, &v_at_reset);
    out.first_state = x;
    // frame 2
    const auto second = front_end(g_source);
    imu::build_measurement_window(buffer, last_reset, t1, window);
    integ.integrate_batch(window);
    const imu::State predicted = hand_predict(P, integ, x, R_at_reset, v_at_reset);
    const M15 predicted_covariance = alg::lio::transform_covariance_imu_to_lidar(integ.get_raw().covariance, P.imu.T_imu_to_lidar, predicted.rotation);
    {  // is the IMU prior the one the alignment will use? (what sp_lio_stepper_create decides from the same covariance)
        M15 H;
        Eigen::Matrix<float, 15, 1> b;
        out.prior_valid = imu::compute_imu_hessian_gradient(predicted, predicted, predicted_covariance, H, b);
    }
    PointCloudShared sampled(q);
    const PointCloudShared* source = second.get();
    if (P.registration_sampling.enable && second->size() > P.registration_sampling.num) {
        proc.random_sampling(*second, sampled, P.registration_sampling.num);
        source = &sampled;
    }
    auto result = registration.align(*source, submap.get_submap_point_cloud(), submap.get_submap_kdtree(), predicted, predicted_covariance,
                                     P_post, hand_observable(P, window), static_cast<float>(t1 - t0), odom.matrix());
    x = result.state;
    throw_on_error(sp_lio_clamp_bias_host(x.accel_bias.data(), P.lio.bias_estimation.max_accel_bias));
    throw_on_error(sp_lio_clamp_bias_host(x.gyro_bias.data(), P.lio.bias_estimation.max_gyro_bias));
    P_post = result.posterior_covariance;
    hand_reset(P, integ, x, P_post, &R_at_reset, &v_at_reset);
    out.pose = result.registration_result.T.matrix();
    out.state = x;
    out.P_post = P_post;
    out.rows_first = first->size();
    out.rows_second = second->size();
    out.inlier = result.registration_result.inlier;
    out.iterations = result.registration_result.iterations;
    return out;
}

// what case 3 compares a rejected-then-accepted first frame with
static imu::State g_first_state;
static M4 g_first_odom = M4::Identity();
static size_t g_rows_first = 0, g_first_submap = 0;
static float g_hand_spread = 0.0f;
static bool g_hand_identical = false;

static void pipeline_is_the_chain() {
    const HandResult a = hand_chain(), b = hand_chain();
    g_hand_spread = std::max({max_entry_diff(a.pose, b.pose), state_diff(a.state, b.state), max_diff(a.P_post.data(), b.P_post.data(), 225)});
    g_hand_identical = std::memcmp(a.pose.data(), b.pose.data(), 16 * sizeof(float)) == 0 && same_state(a.state, b.state) &&
                       std::memcmp(a.P_post.data(), b.P_post.data(), 225 * sizeof(float)) == 0;
    std::printf("  hand chain: rows %zu / %zu, inliers %u, iterations %zu, IMU prior %s; second run rows %zu / %zu, inliers %u; largest entry "
                "difference %.3g (%s)\n", a.rows_first, a.rows_second, a.inlier, a.iterations, a.prior_valid ? "valid" : "INVALID", b.rows_first,
                b.rows_second, b.inlier, g_hand_spread, g_hand_identical ? "bit-identical" : "NOT bit-identical");
    print_pose("hand chain pose", a.pose);
    print_state("hand chain state", a.state);
    CHECK(a.rows_first == b.rows_first && a.rows_second == b.rows_second);
    CHECK(a.prior_valid);  // (the shared settings are meant to run the IMU prior; case 6 runs without it)

    Pipeline p(shared_params());
    feed(p, 180, 240, resting);
    const Result r0 = p.process(upload(p, g_target), frame_time(0));
    const size_t rows_first = p.get_preprocessed_point_cloud().size();
    g_first_state = p.get_lio_state();
    g_first_odom = p.get_odom().matrix();
    g_rows_first = rows_first;
    g_first_submap = p.get_submap_point_cloud().size();
    const bool first_covariance_zero = max_diff(p.get_posterior_covariance().data(), M15::Zero().data(), 225) == 0.0f;
    const Result r1 = p.process(upload(p, g_source), frame_time(1));
    const size_t rows_second = p.get_preprocessed_point_cloud().size();
    const M4 pose = p.get_odom().matrix();
    const float d_pose = max_entry_diff(pose, a.pose), d_state = state_diff(p.get_lio_state(), a.state);
    const float d_cov = max_diff(p.get_posterior_covariance().data(), a.P_post.data(), 225);
    const float bound = g_hand_identical ? 0.0f : 4.0f * g_hand_spread;
    std::printf("  pipeline: results %d, %d; rows %zu / %zu; inliers %u; message '%s'\n", int(r0), int(r1), rows_first, rows_second,
                p.get_registration_result().inlier, p.get_error_message().c_str());
    print_pose("pipeline pose", pose);
    print_state("pipeline state", p.get_lio_state());
    std::printf("  |pipeline - hand|: pose %.3g, state %.3g, posterior covariance %.3g; bound %.3g\n", d_pose, d_state, d_cov, bound);
    CHECK(r0 == Result::first_frame);
    CHECK(r1 == Result::success);
    CHECK(first_covariance_zero);
    CHECK(same_state(g_first_state, a.first_state));
    CHECK(rows_first == a.rows_first && rows_second == a.rows_second);
    if (g_hand_identical) {
        CHECK(std::memcmp(pose.data(), a.pose.data(), 16 * sizeof(float)) == 0);
        CHECK(same_state(p.get_lio_state(), a.state));
        CHECK(std::memcmp(p.get_posterior_covariance().data(), a.P_post.data(), 225 * sizeof(float)) == 0);
    } else {
        CHECK(d_pose <= bound);
        CHECK(d_state <= bound);
        CHECK(d_cov <= bound);
    }
    CHECK(p.get_registration_result().inlier == a.inlier || !g_hand_identical);
    CHECK(max_entry_diff(pose, pose_of(p.get_lio_state())) == 0.0f);  // odom_ == state_to_pose(x_)
    CHECK(max_entry_diff(p.get_prev_odom().matrix(), M4::Identity()) == 0.0f);
    CHECK(p.get_keyframe_poses().size() == 1);
    // the second frame's stage times: one run, not warmed up
    for (const auto& [key, us] : p.get_current_processing_time()) std::printf("  %-24s %10.1f us\n", key.c_str(), us);
}

// ------------------------------------------------------------------------------------------------ 2. a drive from rest
static constexpr int kFrames = 5;
static std::vector<PointCloudCPU> g_drive;
static const std::vector<PointCloudCPU>& drive_frames() {
    if (g_drive.empty())
        for (int k = 0; k < kFrames; ++k) g_drive.push_back(seen_from(g_target, drive_pose(frame_time(k))));
    return g_drive;
}
static void check_pair(const char* label, int from, int to, const M4& pose_from, const M4& pose_to, bool assert_bound) {
    float dt, dr;
    pose_error(relative(pose_from, pose_to), relative(drive_pose(frame_time(from)), drive_pose(frame_time(to))), &dt, &dr);
    std::printf("  %s: frames %d -> %d: relative translation error %.4f m (bound %.2f), rotation entry error %.5f (bound %.2f)%s\n", label, from,
                to, dt, kTransBound, dr, kRotBound, assert_bound ? "" : " [printed only]");
    if (assert_bound) {
        CHECK(dt <= kTransBound);
        CHECK(dr <= kRotBound);
    }
}
static void drive(const char* label, const lio::Parameters& params) {
    const auto& frames = drive_frames();
    Pipeline p(params);
    std::vector<M4> poses;
    for (int k = 0; k < kFrames; ++k) {
        feed_until_frame(p, k);
        const Result r = p.process(upload(p, frames[k]), frame_time(k));
        poses.push_back(p.get_odom().matrix());
        std::printf("  %s: frame %d result %d, inliers %u, iterations %zu, submap %zu points, keyframes %zu, message '%s'\n", label, k, int(r),
                    p.get_registration_result().inlier, p.get_registration_result().iterations, p.get_submap_point_cloud().size(),
                    p.get_keyframe_poses().size(), p.get_error_message().c_str());
        CHECK(r == (k == 0 ? Result::first_frame : Result::success));
        if (k > 0) check_pair(label, k - 1, k, poses[k - 1], poses[k], true);
    }
    const imu::State& x = p.get_lio_state();
    const double s = frame_time(kFrames - 1) - 1.0;
    const V3 v_true(float(kAccel * s), 0.0f, 0.0f);
    const float v_err = (x.velocity - v_true).norm();
    print_state(label, x);
    std::printf("  %s: final velocity error %.4f m/s (true %.2f m/s in x; bound %.2f), |b_a| = %.3g, |b_g| = %.3g\n", label, v_err, v_true[0],
                kTransBound / float(kFramePeriod), x.accel_bias.norm(), x.gyro_bias.norm());
    CHECK(v_err <= kTransBound / float(kFramePeriod));
    CHECK(max_entry_diff(poses.back(), pose_of(x)) == 0.0f);
}
static lio::Parameters voxel_hash_map_params() {
    lio::Parameters params = shared_params();
    params.submap.map_type = od::SubmapMapType::VOXEL_HASH_MAP;
    params.submap.keyframe.distance_threshold = 0.1f;  // the drive covers 0.32 m
    params.submap.keyframe.angle_threshold_degrees = 1e3f;
    params.submap.keyframe.time_threshold_seconds = 1e6f;
    params.submap.keyframe.inlier_ratio_threshold = 0.0f;
    return params;
}
static void drive_from_rest() {
    drive("occupancy grid", shared_params());
    drive("voxel hash map", voxel_hash_map_params());
}

// ------------------------------------------------------------------------------------------------ 3. IMU only
static void imu_only() {
    const auto& frames = drive_frames();
    const lio::Parameters params = shared_params();
    {
        Pipeline p(params);
        const lio::Parameters& P = p.get_params();
        std::vector<M4> poses;
        for (int k = 0; k < kFrames; ++k) {
            feed_until_frame(p, k);
            if (k != 3) {
                const Result r = p.process(upload(p, frames[k]), frame_time(k));
                poses.push_back(p.get_odom().matrix());
                CHECK(r == (k == 0 ? Result::first_frame : Result::success));
                continue;
            }
            // frame 3: 50 points. The window [t2, t3] integrated by hand from the state and covariance read before the call
            const imu::State before = p.get_lio_state();
            const M15 P_before = p.get_posterior_covariance();
            const M4 odom_before = p.get_odom().matrix();
            imu::IMUPreintegration integ(P.imu.preintegration);
            M3 R_at_reset;
            V3 v_at_reset;
            hand_reset(P, integ, before, P_before, &R_at_reset, &v_at_reset);
            std::vector<imu::IMUMeasurement> window;
            imu::build_measurement_window(p.get_imu_buffer(), frame_time(2), frame_time(3), window);
            integ.integrate_batch(window);
            const imu::State predicted = hand_predict(P, integ, before, R_at_reset, v_at_reset);
            const M15 predicted_covariance = alg::lio::transform_covariance_imu_to_lidar(integ.get_raw().covariance, P.imu.T_imu_to_lidar, predicted.rotation);

            const PointCloudCPU small = subset(frames[3], 50);
            CHECK(small.size() == 50);
            const Result r = p.process(upload(p, small), frame_time(3));
            poses.push_back(p.get_odom().matrix());
            const auto& reg = p.get_registration_result();
            std::printf("  frame 3: result %d, message '%s', preprocessed %zu points, window %zu samples\n", int(r), p.get_error_message().c_str(),
                        p.get_preprocessed_point_cloud().size(), window.size());
            print_state("state before", before);
            print_state("hand prediction", predicted);
            print_state("pipeline state", p.get_lio_state());
            std::printf("  |state - hand| = %.3g, |P_post - hand| = %.3g\n", state_diff(p.get_lio_state(), predicted),
                        max_diff(p.get_posterior_covariance().data(), predicted_covariance.data(), 225));
            CHECK(r == Result::imu_only);
            CHECK(p.get_error_message() == "point cloud size is too small; propagated with IMU only");
            CHECK(p.get_preprocessed_point_cloud().size() <= P.registration.min_num_points);
            CHECK(window.size() >= 20);
            CHECK(same_state(p.get_lio_state(), predicted));
            CHECK(std::memcmp(poses.back().data(), pose_of(predicted).data(), 16 * sizeof(float)) == 0);
            CHECK(std::memcmp(p.get_posterior_covariance().data(), predicted_covariance.data(), 225 * sizeof(float)) == 0);
            CHECK(max_entry_diff(p.get_prev_odom().matrix(), odom_before) == 0.0f);
            CHECK(max_entry_diff(reg.T.matrix(), poses.back()) == 0.0f);
            CHECK(reg.converged && reg.iterations == 0 && reg.inlier == 0 && reg.error == 0.0f && reg.error_raw == 0.0f);
            CHECK(max_diff(reg.H.data(), Eigen::Matrix<float, 6, 6>::Zero().data(), 36) == 0.0f && max_diff(reg.b.data(), Eigen::Matrix<float, 6, 1>::Zero().data(), 6) == 0.0f);
            CHECK(max_diff(reg.H_raw.data(), Eigen::Matrix<float, 6, 6>::Zero().data(), 36) == 0.0f && max_diff(reg.b_raw.data(), Eigen::Matrix<float, 6, 1>::Zero().data(), 6) == 0.0f);
            check_pair("IMU only", 2, 3, poses[2], poses[3], false);
        }
        // frame 4, a full scan again: registered against the map, inside the drive's bound of the truth from the last registered frame
        check_pair("after IMU only", 3, 4, poses[3], poses[4], false);
        check_pair("after IMU only", 2, 4, poses[2], poses[4], true);
        CHECK(p.get_registration_result().iterations > 0 && p.get_registration_result().inlier > 0);
    }
    {  // a too small FIRST frame is rejected before the integrator is touched; the next full frame is the first frame of case 1
        Pipeline p(params);
        feed(p, 180, 240, resting);
        const PointCloudCPU small = subset(g_target, 50);
        CHECK(small.size() == 50);
        const Result r = p.process(upload(p, small), frame_time(0));
        std::printf("  small first frame: result %d, message '%s'\n", int(r), p.get_error_message().c_str());
        CHECK(r == Result::small_number_of_points);
        CHECK(p.get_error_message() == "point cloud size is too small");
        CHECK(p.process(upload(p, g_target), frame_time(0)) == Result::first_frame);  // (nothing was accepted before: the same stamp is not old)
        CHECK(same_state(p.get_lio_state(), g_first_state));
        CHECK(std::memcmp(p.get_odom().matrix().data(), g_first_odom.data(), 16 * sizeof(float)) == 0);
        CHECK(max_diff(p.get_posterior_covariance().data(), M15::Zero().data(), 225) == 0.0f);
        CHECK(p.get_preprocessed_point_cloud().size() == g_rows_first && p.get_submap_point_cloud().size() == g_first_submap);
        CHECK(g_rows_first > 0);  // (case 1 ran)
    }
}

// ------------------------------------------------------------------------------------------------ 4. result codes
static PointCloudCPU stamped(const PointCloudCPU& cloud, double start_sec) {
    PointCloudCPU c = cloud;
    c.timestamp_offsets->resize(c.size());
    for (size_t i = 0; i < c.size(); ++i) (*c.timestamp_offsets)[i] = 100.0f * float(i) / float(c.size());
    c.start_time_ms = start_sec * 1e3;
    c.end_time_ms = start_sec * 1e3 + 100.0;
    return c;
}
static void result_codes() {
    {  // a stamp that does not advance; the timing keys
        Pipeline p(shared_params());
        feed(p, 180, 240, resting);
        CHECK(p.process(upload(p, g_target), frame_time(0)) == Result::first_frame);
        CHECK(p.get_error_message().empty());
        CHECK(p.process(upload(p, g_target), frame_time(0)) == Result::old_timestamp);
        CHECK(p.get_error_message() == "old timestamp");
        CHECK(p.process(upload(p, g_target), 0.5) == Result::old_timestamp);
        CHECK(p.process(upload(p, g_target), frame_time(1)) == Result::success);
        CHECK(p.get_error_message().empty());
        const auto& cur = p.get_current_processing_time();
        const auto& tot = p.get_total_processing_times();
        for (const char* key : {"1. preprocessing", "2. compute covariances", "3. lio registration", "4. build submap"}) {
            CHECK(cur.count(key) == 1 && cur.at(key) > 0.0);
            CHECK(tot.count(key) == 1 && !tot.at(key).empty());
            if (cur.count(key)) std::printf("  %-24s %10.1f us\n", key, cur.at(key));
        }
        CHECK(cur.size() == 4 && tot.size() == 4);
        CHECK(tot.at("1. preprocessing").size() == 2 && tot.at("3. lio registration").size() == 1);
    }
    {  // a stage that reports an argument error: the IMU deskew refuses a scan without a queue, before it launches anything
        lio::Parameters params = shared_params();
        params.imu.deskew.enable = true;
        Pipeline p(params);
        feed(p, 180, 240, resting);
        auto scan = upload(p, stamped(g_target, frame_time(0)));
        scan->queue.ptr.reset();
        CHECK(p.process(scan, frame_time(0)) == Result::error);
        std::printf("  error message: '%s'\n", p.get_error_message().c_str());
        CHECK(p.get_error_message().rfind("preprocess: ", 0) == 0);
        CHECK(p.get_error_message().find("queue is not initialized") != std::string::npos);
        CHECK(p.process(upload(p, stamped(g_target, frame_time(0))), frame_time(0)) == Result::first_frame);  // nothing was accepted before
    }
    CHECK(int(Result::success) == 0 && int(Result::first_frame) == 1 && int(Result::waiting_initial_alignment) == 2 && int(Result::imu_only) == 3 &&
          int(Result::error) == 100 && int(Result::old_timestamp) == 101 && int(Result::small_number_of_points) == 102);
}

// ------------------------------------------------------------------------------------------------ 5. / 6. at rest
/// the same scan twice with an IMU at rest that reads the parameters' biases on top of (0, 0, g) and 0
static Result two_identical_frames(Pipeline& p) {
    const V3 ba = p.get_params().imu.bias.accel_bias, bg = p.get_params().imu.bias.gyro_bias;
    feed(p, 180, 240, [&](int tick) { return sample(tick_time(tick), bg, V3(ba[0], ba[1], kG + ba[2])); });
    if (p.process(upload(p, g_target), frame_time(0)) != Result::first_frame) return Result::error;
    return p.process(upload(p, g_target), frame_time(1));
}
static void bias_rules() {
    {
        lio::Parameters params = shared_params();
        params.lio.bias_estimation.freeze_on_low_excitation = true;
        params.imu.bias.accel_bias = V3(1e-3f, -2e-3f, 5e-4f);
        params.imu.bias.gyro_bias = V3(1e-4f, 2e-4f, -3e-4f);
        Pipeline p(params);
        const Result r = two_identical_frames(p);
        const imu::State& x = p.get_lio_state();
        const float d = max_entry_diff(p.get_odom().matrix(), M4::Identity());
        print_state("frozen biases", x);
        std::printf("  result %d, |pose - I| = %.3g (bound 1e-4), |v| = %.3g (bound %.3g), message '%s'\n", int(r), d, x.velocity.norm(),
                    1e-4f / float(kFramePeriod), p.get_error_message().c_str());
        CHECK(r == Result::success);
        CHECK(std::memcmp(x.accel_bias.data(), params.imu.bias.accel_bias.data(), 3 * sizeof(float)) == 0);
        CHECK(std::memcmp(x.gyro_bias.data(), params.imu.bias.gyro_bias.data(), 3 * sizeof(float)) == 0);
        CHECK(d <= 1e-4f);
        CHECK(x.velocity.norm() <= 1e-4f / float(kFramePeriod));
    }
    {  // the clamp: a gyro bias of 0.02 rad/s with max_gyro_bias 0.01
        lio::Parameters params = shared_params();
        params.lio.bias_estimation.freeze_on_low_excitation = true;
        params.imu.bias.gyro_bias = V3(0.02f, 0.0f, 0.0f);
        params.lio.bias_estimation.max_gyro_bias = 0.01f;
        Pipeline p(params);
        const Result r = two_identical_frames(p);
        const imu::State& x = p.get_lio_state();
        print_state("clamped gyro bias", x);
        std::printf("  result %d, |b_g| = %.9g (limit 0.01)\n", int(r), x.gyro_bias.norm());
        CHECK(r == Result::success);
        CHECK(x.gyro_bias.norm() <= 0.01f * (1.0f + 4.0f * 1.1920929e-7f));
        CHECK(x.gyro_bias.norm() >= 0.005f && x.gyro_bias[0] > 0.0f);  // clamped, not zeroed
    }
}
static void invalid_prior() {
    lio::Parameters params = shared_params();
    params.lio.bias_estimation.freeze_on_low_excitation = true;
    params.imu.preintegration = imu::IMUPreintegrationParams();  // all four densities 0: the predicted covariance is singular
    Pipeline p(params);
    const Result r = two_identical_frames(p);
    const imu::State& x = p.get_lio_state();
    float v[21];
    pack(x, v);
    const float d = max_entry_diff(p.get_odom().matrix(), M4::Identity());
    print_state("invalid prior", x);
    std::printf("  result %d, |pose - I| = %.3g (bound 1e-4), inliers %u, iterations %zu, largest |P_post| %.3g, message '%s'\n", int(r), d,
                p.get_registration_result().inlier, p.get_registration_result().iterations,
                max_diff(p.get_posterior_covariance().data(), M15::Zero().data(), 225), p.get_error_message().c_str());
    CHECK(r == Result::success);
    CHECK(all_finite(v, 21));
    CHECK(all_finite(p.get_posterior_covariance().data(), 225));
    CHECK(d <= 1e-4f);
}

// ------------------------------------------------------------------------------------------------ 7. initial alignment
static void initial_alignment() {
    const float roll = 10.0f * kPi / 180.0f, pitch = -5.0f * kPi / 180.0f, yaw_user = 30.0f * kPi / 180.0f;
    // the specific force of a device at rest with R_world_body = Ry(pitch) Rx(roll): R^T (0, 0, g)
    const V3 force(-std::sin(pitch) * kG, std::cos(pitch) * std::sin(roll) * kG, std::cos(pitch) * std::cos(roll) * kG);
    const V3 gyro(0.002f, -0.001f, 0.003f);
    lio::Parameters params = shared_params();
    params.imu.initial_alignment.enable = true;
    params.imu.enable = false;  // (the struct's default: the constructor forces it)
    params.pose.initial.matrix() = rigid(yaw_user, 1.0f, 2.0f, 3.0f);
    Pipeline p(params);
    std::printf("  imu.enable %d, buffer_duration_sec %.3f\n", int(p.get_params().imu.enable), p.get_params().imu.buffer_duration_sec);
    CHECK(p.get_params().imu.enable);
    CHECK(std::fabs(p.get_params().imu.buffer_duration_sec - 1.2) < 1e-6);
    auto tilted = [&](int tick) { return sample(tick_time(tick), gyro, force); };
    feed(p, 1900, 2000, tilted);  // 9.5 .. 10.0: 0.5 s < required_duration_sec
    CHECK(p.process(upload(p, g_target), tick_time(2000)) == Result::waiting_initial_alignment);
    std::printf("  message: '%s'\n", p.get_error_message().c_str());
    CHECK(p.get_error_message() == "initial_alignment: IMU buffer spans less than required_duration_sec");
    CHECK(max_entry_diff(p.get_odom().matrix(), rigid(yaw_user, 1.0f, 2.0f, 3.0f)) == 0.0f);
    feed(p, 2001, 2140, tilted);  // .. 10.7
    const Result r = p.process(upload(p, g_target), tick_time(2140));
    const M4 odom = p.get_odom().matrix();
    print_pose("odom after the alignment", odom);
    CHECK(r == Result::first_frame);
    // the estimator by hand on the same buffer, the user's yaw layered on the left
    imu::InitialAlignmentEstimator estimator(params.imu.initial_alignment, params.imu.preintegration.gravity, params.imu.T_imu_to_lidar);
    const auto out = estimator.try_align(tick_time(2140), p.get_imu_buffer(), params.imu.bias);
    CHECK(out.status == imu::InitialAlignmentEstimator::Status::success);
    const M3 expect = Eigen::AngleAxisf(imu::detail::yaw_from_rotation(params.pose.initial.rotation()), V3(0.0f, 0.0f, 1.0f)).toRotationMatrix() *
                      out.R_gravity_lidar;
    const imu::State& x = p.get_lio_state();
    const M3 R_odom = iso(odom).rotation();
    std::printf("  roll %.6f (true %.6f), pitch %.6f (true %.6f); |R_odom - Rz(yaw) R_gravity_lidar| = %.3g; gyro bias (%.4g %.4g %.4g)\n",
                out.roll_rad, roll, out.pitch_rad, pitch, max_diff(R_odom.data(), expect.data(), 9), x.gyro_bias[0], x.gyro_bias[1], x.gyro_bias[2]);
    CHECK(std::memcmp(R_odom.data(), expect.data(), 9 * sizeof(float)) == 0);
    CHECK(std::memcmp(x.rotation.data(), expect.data(), 9 * sizeof(float)) == 0);
    CHECK(std::memcmp(x.gyro_bias.data(), out.gyro_bias.data(), 3 * sizeof(float)) == 0);
    CHECK(std::fabs(x.gyro_bias[0] - gyro[0]) <= 1e-6f && std::fabs(x.gyro_bias[1] - gyro[1]) <= 1e-6f && std::fabs(x.gyro_bias[2] - gyro[2]) <= 1e-6f);
    CHECK(std::fabs(out.roll_rad - roll) <= 1e-5f && std::fabs(out.pitch_rad - pitch) <= 1e-5f);
    for (int j = 0; j < 3; ++j) CHECK(std::fabs(odom(2, j) - force[j] / kG) <= 1e-5f);  // the tilt itself: the third row is the force's direction
    CHECK(odom(0, 3) == 1.0f && odom(1, 3) == 2.0f && odom(2, 3) == 3.0f);
    CHECK(x.position[0] == 1.0f && x.position[1] == 2.0f && x.position[2] == 3.0f && x.velocity.norm() == 0.0f);
    CHECK(max_entry_diff(p.get_keyframe_poses().front().matrix(), odom) == 0.0f);  // the first keyframe is anchored at the aligned pose
}

// ------------------------------------------------------------------------------------------------ 8. the deskew
static void deskew_uses_state() {
    lio::Parameters params = shared_params();
    params.imu.deskew.enable = true;
    Pipeline p(params);
    const lio::Parameters& P = p.get_params();
    feed(p, 180, 280, resting);  // 0.9 .. 1.4: both scans and the deskew's margin
    Result results[2];
    for (int k = 0; k < 2; ++k) {
        const PointCloudCPU cpu = stamped(g_target, frame_time(k));
        // the deskew by hand on a copy, with the state read before the call (deskew_with_imu's arguments, pointcloud_processing.hpp:103-112)
        const imu::State before = p.get_lio_state();
        PointCloudShared by_hand(*p.get_device_queue(), cpu);
        alg::deskew::IMUDeskewStatus status;
        const M3 R_world_imu = p.get_odom().rotation() * P.imu.T_imu_to_lidar.rotation();
        const bool ok = alg::deskew::deskew_point_cloud_imu(by_hand, by_hand, p.get_imu_buffer(), by_hand.start_time_ms * 1e-3, P.imu.T_imu_to_lidar,
                                                           imu::IMUBias{before.gyro_bias, before.accel_bias}, P.imu.preintegration, R_world_imu,
                                                           before.velocity, &status, P.imu.deskew.gyro_only);
        CHECK(ok && status == alg::deskew::IMUDeskewStatus::success);
        auto scan = upload(p, cpu);
        results[k] = p.process(scan, frame_time(k));
        const size_t n = scan->size();
        const bool in_place = n == cpu.size() && n == by_hand.size() && std::memcmp(scan->points->data(), by_hand.points->data(), n * sizeof(PointType)) == 0;
        size_t moved = 0;
        float farthest = 0.0f;
        for (size_t i = 0; i < n && i < cpu.size(); ++i) {
            const float d = max_diff(scan->points->data()[i].data(), (*cpu.points)[i].data(), 3);
            moved += d > 0.0f;
            farthest = std::max(farthest, d);
        }
        std::printf("  frame %d: result %d, the caller's scan %s the hand deskew; %zu of %zu points differ from the raw scan, by at most %.3g m; message '%s'\n",
                    k, int(results[k]), in_place ? "equals" : "DIFFERS FROM", moved, n, farthest, p.get_error_message().c_str());
        CHECK(in_place);
        CHECK(scan->has_timestamps());
        CHECK(farthest <= 1e-3f);  // at rest nothing moves
    }
    const float d = max_entry_diff(p.get_odom().matrix(), M4::Identity());
    std::printf("  |pose - I| = %.3g (bound 1e-4)\n", d);
    CHECK(results[0] == Result::first_frame && results[1] == Result::success);
    CHECK(d <= 1e-4f);
    CHECK(p.get_preprocessed_point_cloud().size() > 1000 && p.get_preprocessed_point_cloud().has_timestamps());
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <golden dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    g_target = PointCloudReader::readFile(dir + "/target.ply");
    g_source = PointCloudReader::readFile(dir + "/source.ply");
    if (g_target.size() == 0 || g_source.size() == 0) { std::printf("cannot read the golden files in %s\n", dir.c_str()); return 2; }
    std::printf("target %zu points (intensity %d), source %zu points\n", g_target.size(), int(g_target.has_intensity()), g_source.size());
    RUN(pipeline_is_the_chain);
    RUN(drive_from_rest);
    RUN(imu_only);
    RUN(result_codes);
    RUN(bias_rules);
    RUN(invalid_prior);
    RUN(initial_alignment);
    RUN(deskew_uses_state);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
