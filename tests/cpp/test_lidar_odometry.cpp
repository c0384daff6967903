// C++ tests of pipeline::lidar_odometry::LiDAROdometryPipeline, included through the reference's paths only. Built and run by
// tests/test_gpu_lidar_odometry.py on a GPU box: test_lidar_odometry <golden dir>; exit code 0 = all checks passed.
//   1. the pipeline is the chain: target.ply at t = 0.0 and source.ply at t = 0.1 through process() against the same calls made by
//      hand with fresh objects (bit for bit when two hand runs agree bit for bit, else within four times their difference)
//   2. that pose against the bundled ground truth (0.05 m, 0.01 per rotation entry)
//   3. a drive of five frames with both submap types: relative motion, keyframe counts, the submap's size
//   4. result codes, messages and the four timing keys
//   5. the IMU paths: buffer rules, the initial-alignment gate, the three motion-prediction modes, the velocity-update switch;
//      the IMU deskew in preprocess and the velocity update on a stamped scan at rest
// Every figure is printed before it is checked.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sycl_points/algorithms/common/transform.hpp"
#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/intensity_correction.hpp"
#include "sycl_points/algorithms/filter/polar_downsampling.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/registration/registration_pipeline.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"
#include "sycl_points/pipeline/lidar_odometry.hpp"

using namespace sycl_points;
namespace alg = sycl_points::algorithms;
namespace lo = sycl_points::pipeline::lidar_odometry;
namespace od = sycl_points::pipeline::odometry;
using Pipeline = lo::LiDAROdometryPipeline;
using Result = Pipeline::ResultType;
using V3 = Eigen::Vector3f;
using M3 = Eigen::Matrix3f;
using M4 = Eigen::Matrix4f;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); std::fflush(stdout); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); std::fflush(stdout); } while (0)

static constexpr float kPi = 3.14159265358979323846f;
static constexpr float kTransBound = 0.05f, kRotBound = 0.01f;  // tests/test_gpu_facade.py's bound on this pair
static PointCloudCPU g_target, g_source;
static M4 g_T_gt = M4::Identity();
static float g_hand_spread = 0.0f;  // the largest entry difference between two hand runs of the chain (0: bit-identical)
static M4 g_pipeline_pose = M4::Identity();

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
static float max_entry_diff(const M4& A, const M4& B) {
    float d = 0.0f;
    for (int k = 0; k < 16; ++k) d = std::max(d, std::fabs(A.data()[k] - B.data()[k]));
    return d;
}
static void pose_error(const M4& T, const M4& ref, float* trans, float* rot) {
    const float dx = T(0, 3) - ref(0, 3), dy = T(1, 3) - ref(1, 3), dz = T(2, 3) - ref(2, 3);
    *trans = std::sqrt(dx * dx + dy * dy + dz * dz);
    *rot = 0.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) *rot = std::max(*rot, std::fabs(T(i, j) - ref(i, j)));
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
static PointCloudShared::Ptr upload(const Pipeline& p, const PointCloudCPU& cpu) {
    return std::make_shared<PointCloudShared>(*p.get_device_queue(), cpu);
}
static lo::Parameters defaults_without_imu() {
    lo::Parameters p;
    p.imu.enable = false;
    return p;
}

// ------------------------------------------------------------------------------------------------ 1. the chain, by hand
struct HandResult {
    M4 pose;
    size_t rows_first, rows_second;
    uint32_t inlier;
};
/// What process() does for two frames with the default parameters and the IMU off, call by call on fresh objects: ONE
/// PreprocessFilter and ONE PolarGrid for both frames (PCProcessor's), robust covariances, the incidence filter, the intensity
/// correction; the first cloud transform-copied to the identity, a KD-tree on it, the covariances Submap::compute_covariances
/// asks for (plain ones when the cloud has none - with the default parameters it brings its own along), and
/// RegistrationPipeline::align from the identity with dt = 0.1.
static HandResult hand_chain() {
    const lo::Parameters P = defaults_without_imu();
    sycl_utils::DeviceQueue q(0);
    alg::filter::PreprocessFilter filter(q);
    alg::filter::PolarGrid polar(q, P.scan.downsampling.polar.distance_size, P.scan.downsampling.polar.elevation_size,
                                 P.scan.downsampling.polar.azimuth_size, alg::coordinate_system_from_string(P.scan.downsampling.polar.coord_system));
    auto preprocess = [&](const PointCloudCPU& cpu) {
        PointCloudShared scan(q, cpu);
        auto pc = std::make_shared<PointCloudShared>(q);
        filter.box_filter(scan, *pc, P.scan.preprocess.box_filter.min, P.scan.preprocess.box_filter.max);
        polar.downsampling(*pc, *pc);
        filter.random_sampling(*pc, P.scan.downsampling.random.num);
        const auto tree = alg::knn::KDTree::build(q, *pc);
        alg::knn::KNNResult knn;
        auto ev = tree->knn_search_async(*pc, P.covariance_estimation.neighbor_num, knn);
        ev += alg::covariance::estimate_robust_async(knn, *pc, P.covariance_estimation.m_estimation.type,
                                                     P.covariance_estimation.m_estimation.mad_scale,
                                                     P.covariance_estimation.m_estimation.min_robust_scale,
                                                     P.covariance_estimation.m_estimation.max_iterations, ev.evs);
        ev.wait_and_throw();
        filter.angle_incidence_filter(*pc, *pc, P.scan.preprocess.angle_incidence_filter.min_angle,
                                      P.scan.preprocess.angle_incidence_filter.max_angle);
        if (pc->has_intensity()) {
            const auto& ic = P.scan.intensity_correction;
            alg::intensity_correction::correct_intensity(*pc, ic.exp, ic.scale, ic.min_intensity, ic.max_intensity, ic.ref_distance, ic.angle_exponent);
        }
        return pc;
    };
    const auto first = preprocess(g_target);
    PointCloudShared submap = alg::transform::transform_copy(*first, M4::Identity());
    const auto submap_tree = alg::knn::KDTree::build(q, submap);
    if (!submap.has_cov()) alg::covariance::estimate_async(*submap_tree, submap, P.covariance_estimation.neighbor_num).wait_and_throw();
    const auto second = preprocess(g_source);
    alg::registration::RegistrationPipeline reg(q, P.make_registration_pipeline_params());
    alg::registration::Registration::ExecutionOptions options;
    options.dt = 0.1f;
    options.prev_pose = M4::Identity();
    const auto result = reg.align(*second, submap, *submap_tree, M4::Identity(), options);
    return HandResult{result.T.matrix(), first->size(), second->size(), result.inlier};
}

static void print_pose(const char* label, const M4& T) {
    std::printf("  %s\n", label);
    for (int r = 0; r < 4; ++r) std::printf("    % .9g % .9g % .9g % .9g\n", T(r, 0), T(r, 1), T(r, 2), T(r, 3));
}

static void pipeline_is_the_chain() {
    const HandResult a = hand_chain(), b = hand_chain();
    g_hand_spread = max_entry_diff(a.pose, b.pose);
    const bool identical = std::memcmp(a.pose.data(), b.pose.data(), 16 * sizeof(float)) == 0;
    std::printf("  hand chain: rows %zu / %zu, inliers %u; second run rows %zu / %zu, inliers %u; largest entry difference %.3g (%s)\n",
                a.rows_first, a.rows_second, a.inlier, b.rows_first, b.rows_second, b.inlier, g_hand_spread,
                identical ? "bit-identical" : "NOT bit-identical");
    print_pose("hand chain pose", a.pose);
    CHECK(a.rows_first == b.rows_first && a.rows_second == b.rows_second);

    Pipeline p(defaults_without_imu());
    const Result r0 = p.process(upload(p, g_target), 0.0);
    const size_t rows_first = p.get_preprocessed_point_cloud().size();
    const Result r1 = p.process(upload(p, g_source), 0.1);
    const size_t rows_second = p.get_preprocessed_point_cloud().size();
    g_pipeline_pose = p.get_odom().matrix();
    const float diff = max_entry_diff(g_pipeline_pose, a.pose);
    const float bound = identical ? 0.0f : 4.0f * g_hand_spread;
    std::printf("  pipeline: results %d, %d; rows %zu / %zu; inliers %u; message '%s'\n", int(r0), int(r1), rows_first, rows_second,
                p.get_registration_result().inlier, p.get_error_message().c_str());
    print_pose("pipeline pose", g_pipeline_pose);
    std::printf("  |pipeline - hand| = %.3g, bound %.3g\n", diff, bound);
    CHECK(r0 == Result::first_frame);
    CHECK(r1 == Result::success);
    CHECK(rows_first == a.rows_first && rows_second == a.rows_second);
    if (identical) CHECK(std::memcmp(g_pipeline_pose.data(), a.pose.data(), 16 * sizeof(float)) == 0);
    else CHECK(diff <= bound);
    CHECK(p.get_registration_result().inlier == a.inlier || !identical);
    CHECK(max_entry_diff(p.get_prev_odom().matrix(), M4::Identity()) == 0.0f);
    CHECK(p.get_keyframe_poses().size() == 1);
    CHECK(p.get_registration_input_point_cloud() != nullptr && p.get_registration_input_point_cloud()->size() == 1000);
}

// ------------------------------------------------------------------------------------------------ 2. ground truth
static lo::Parameters configuration_1() {  // examples/example_registration.cpp's settings, as far as the pipeline has them
    lo::Parameters p = defaults_without_imu();
    p.scan.preprocess.box_filter.min = 0.5f;
    p.scan.downsampling.polar.enable = false;
    p.scan.downsampling.voxel.enable = true;
    p.scan.downsampling.voxel.size = 0.25f;
    p.scan.downsampling.random.enable = false;
    p.covariance_estimation.m_estimation.enable = false;
    p.registration.factor.robust.type = alg::robust::RobustLossType::GEMAN_MCCLURE;
    p.registration.factor.robust.default_scale = 10.0f;
    p.lo.registration.max_iterations = 10;
    p.lo.registration.optimization.optimization_method = alg::registration::OptimizationMethod::LEVENBERG_MARQUARDT;
    p.lo.pipeline.robust.auto_scale = true;
    p.lo.pipeline.robust.init_scale = 10.0f;
    p.lo.pipeline.robust.min_scale = 2.5f;
    p.lo.pipeline.robust.rotation_init_scale = 5.0f;
    p.lo.pipeline.robust.rotation_min_scale = 2.5f;
    p.lo.pipeline.robust.auto_scaling_iter = 3;
    return p;
}
static void ground_truth() {
    float dt, dr;
    pose_error(g_pipeline_pose, g_T_gt, &dt, &dr);
    std::printf("  odometry defaults: |t - t_gt| = %.4f m (bound %.2f), largest rotation entry difference %.5f (bound %.2f)\n", dt, kTransBound, dr, kRotBound);
    if (!(dt <= kTransBound && dr <= kRotBound)) {  // the figures of the example's settings beside them
        Pipeline p(configuration_1());
        p.process(upload(p, g_target), 0.0);
        p.process(upload(p, g_source), 0.1);
        float dt1, dr1;
        pose_error(p.get_odom().matrix(), g_T_gt, &dt1, &dr1);
        std::printf("  configuration 1: |t - t_gt| = %.4f m, largest rotation entry difference %.5f\n", dt1, dr1);
    }
    CHECK(dt <= kTransBound);
    CHECK(dr <= kRotBound);
}

// ------------------------------------------------------------------------------------------------ 3. a drive
static constexpr int kFrames = 5;
static std::vector<PointCloudCPU> g_drive;
static M4 drive_pose(int k) { return rigid(float(k) * kPi / 180.0f, 0.3f * float(k)); }

/// the five frames through a pipeline: the odometry poses, the submap's size after each frame, the results
struct DriveRun {
    std::vector<M4> poses;
    std::vector<size_t> submap_sizes;
    std::vector<Result> results;
    size_t keyframes = 0;
};
static DriveRun drive(const lo::Parameters& params) {
    if (g_drive.empty())
        for (int k = 0; k < kFrames; ++k) g_drive.push_back(seen_from(g_target, drive_pose(k)));
    DriveRun run;
    Pipeline p(params);
    for (int k = 0; k < kFrames; ++k) {
        run.results.push_back(p.process(upload(p, g_drive[k]), 1.0 + 0.1 * k));  // (a first stamp of 0.0 would read as "no frame yet")
        run.poses.push_back(p.get_odom().matrix());
        run.submap_sizes.push_back(p.get_submap_point_cloud().size());
    }
    run.keyframes = p.get_keyframe_poses().size();
    return run;
}
static void check_relative_motion(const char* label, const DriveRun& run) {
    float dts[kFrames] = {0}, drs[kFrames] = {0};
    bool ok = true;
    for (int k = 1; k < kFrames; ++k) {
        pose_error(relative(run.poses[k - 1], run.poses[k]), relative(drive_pose(k - 1), drive_pose(k)), &dts[k], &drs[k]);
        ok = ok && dts[k] <= kTransBound && drs[k] <= kRotBound;
    }
    std::printf("  %s: results", label);
    for (Result r : run.results) std::printf(" %d", int(r));
    std::printf("; relative translation errors");
    for (int k = 1; k < kFrames; ++k) std::printf(" %.4f", dts[k]);
    std::printf(" m; rotation entry errors");
    for (int k = 1; k < kFrames; ++k) std::printf(" %.5f", drs[k]);
    std::printf("; submap sizes");
    for (size_t s : run.submap_sizes) std::printf(" %zu", s);
    std::printf("; keyframes %zu\n", run.keyframes);
    CHECK(run.results[0] == Result::first_frame);
    for (int k = 1; k < kFrames; ++k) {
        CHECK(run.results[k] == Result::success);
        CHECK(dts[k] <= kTransBound);
        CHECK(drs[k] <= kRotBound);
    }
    (void)ok;
}
static void drive_occupancy_grid() {
    const lo::Parameters params = defaults_without_imu();
    const DriveRun run = drive(params);
    check_relative_motion("occupancy grid", run);
    for (size_t s : run.submap_sizes) CHECK(s >= params.registration.min_num_points);
    CHECK(run.keyframes == 1);  // the occupancy grid takes every frame and declares no keyframe
}
static void drive_voxel_hash_map() {
    lo::Parameters params = defaults_without_imu();
    params.submap.map_type = od::SubmapMapType::VOXEL_HASH_MAP;
    params.submap.keyframe.distance_threshold = 0.5f;
    params.submap.keyframe.angle_threshold_degrees = 1e3f;
    params.submap.keyframe.time_threshold_seconds = 1e6f;
    params.submap.keyframe.inlier_ratio_threshold = 0.0f;
    const DriveRun run = drive(params);
    check_relative_motion("voxel hash map", run);
    CHECK(run.keyframes == 3);  // the start, then 0.6 m and 1.2 m along the way
    for (size_t s : run.submap_sizes) CHECK(s >= params.registration.min_num_points);
    params.submap.keyframe.inlier_ratio_threshold = 1.0f;  // no registration counts as a success: nothing is added
    const DriveRun none = drive(params);
    std::printf("  voxel hash map, inlier_ratio_threshold 1.0: keyframes %zu\n", none.keyframes);
    CHECK(none.keyframes == 1);
    for (int k = 1; k < kFrames; ++k) CHECK(none.results[k] == Result::success);
}

// ------------------------------------------------------------------------------------------------ 4. result codes
static PointCloudCPU first_points(const PointCloudCPU& cloud, size_t n, float min_range) {
    PointCloudCPU out;
    for (size_t i = 0; i < cloud.size() && out.size() < n; i += 97) {
        const PointType& p = (*cloud.points)[i];
        if (std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) > min_range) {
            out.points->push_back(p);
            if (cloud.has_intensity()) out.intensities->push_back((*cloud.intensities)[i]);
        }
    }
    return out;
}
static void result_codes() {
    {  // a stamp that does not advance
        Pipeline p(defaults_without_imu());
        CHECK(p.process(upload(p, g_target), 1.0) == Result::first_frame);
        CHECK(p.get_error_message().empty());
        CHECK(p.process(upload(p, g_source), 1.0) == Result::old_timestamp);
        CHECK(p.get_error_message() == "old timestamp");
        CHECK(p.process(upload(p, g_source), 0.5) == Result::old_timestamp);
        CHECK(p.process(upload(p, g_source), 1.1) == Result::success);
        CHECK(p.get_error_message().empty());
        // the four timing keys, the current frame's and the history's
        const auto& cur = p.get_current_processing_time();
        const auto& tot = p.get_total_processing_times();
        for (const char* key : {"1. preprocessing", "2. compute covariances", "3. registration", "4. build submap"}) {
            CHECK(cur.count(key) == 1 && cur.at(key) > 0.0);
            CHECK(tot.count(key) == 1 && !tot.at(key).empty());
            if (cur.count(key)) std::printf("  %-24s %10.1f us\n", key, cur.at(key));
        }
        CHECK(cur.size() == 4 && tot.size() == 4);
        CHECK(tot.at("1. preprocessing").size() == 2 && tot.at("3. registration").size() == 1);
    }
    {  // 50 points
        Pipeline p(defaults_without_imu());
        const PointCloudCPU small = first_points(g_target, 50, 3.0f);
        CHECK(small.size() == 50);
        CHECK(p.process(upload(p, small), 1.0) == Result::small_number_of_points);
        CHECK(p.get_error_message() == "point cloud size is too small");
        CHECK(p.process(upload(p, g_target), 1.0) == Result::first_frame);  // (nothing was accepted before)
    }
    {  // a stage that throws: the local-mean normalisation refuses mean_min = 0 (intensity_local_mean_norm.hpp:72-74)
        lo::Parameters params = defaults_without_imu();
        params.scan.intensity_local_mean_norm.enable = true;
        params.scan.intensity_local_mean_norm.mean_min = 0.0f;
        Pipeline p(params);
        CHECK(p.process(upload(p, g_target), 1.0) == Result::error);
        std::printf("  error message: '%s'\n", p.get_error_message().c_str());
        CHECK(p.get_error_message().rfind("refine_filter: ", 0) == 0);
        CHECK(p.get_error_message().find("mean_min must be positive") != std::string::npos);
    }
    CHECK(int(Result::success) == 0 && int(Result::first_frame) == 1 && int(Result::waiting_initial_alignment) == 2 &&
          int(Result::error) == 100 && int(Result::old_timestamp) == 101 && int(Result::small_number_of_points) == 102);
}

// ------------------------------------------------------------------------------------------------ 5. IMU paths
static imu::IMUMeasurement sample(double t, const V3& gyro, const V3& accel) {
    imu::IMUMeasurement m;
    m.timestamp = t;
    m.gyro = gyro;
    m.accel = accel;
    return m;
}
static void imu_buffer_rules() {
    const V3 up(0.0f, 0.0f, 9.80665f), zero(0.0f, 0.0f, 0.0f);
    {
        Pipeline p(defaults_without_imu());
        p.add_imu_measurement(sample(0.0, zero, up));
        p.add_imu_measurement(sample(0.01, zero, up));
        CHECK(p.get_imu_buffer().empty());
    }
    lo::Parameters params;
    params.imu.enable = true;
    params.imu.initial_alignment.enable = false;
    params.imu.buffer_duration_sec = 0.5;
    Pipeline p(params);
    const float nan = std::nanf(""), inf = INFINITY;
    p.add_imu_measurement(sample(1.00, zero, up));
    p.add_imu_measurement(sample(1.01, V3(nan, 0.0f, 0.0f), up));
    p.add_imu_measurement(sample(1.02, zero, V3(0.0f, inf, 0.0f)));
    CHECK(p.get_imu_buffer().size() == 1);
    p.add_imu_measurement(sample(1.00, zero, up));  // a duplicate stamp
    p.add_imu_measurement(sample(0.99, zero, up));  // out of order
    CHECK(p.get_imu_buffer().size() == 1);
    bool span_ok = true;
    for (int i = 1; i <= 200; ++i) {
        p.add_imu_measurement(sample(1.0 + 0.01 * i, zero, up));
        const auto buf = p.get_imu_buffer();
        span_ok = span_ok && (buf.back().timestamp - buf.front().timestamp) <= 0.5;
    }
    const auto buf = p.get_imu_buffer();
    std::printf("  buffer: %zu samples, span %.3f s\n", buf.size(), buf.back().timestamp - buf.front().timestamp);
    CHECK(span_ok && buf.size() >= 50 && buf.size() <= 51 && buf.back().timestamp == 1.0 + 0.01 * 200);
    // the constructor widens the buffer for the alignment window; IMU deskew switches the velocity update off
    lo::Parameters q;
    q.imu.enable = true;
    q.imu.buffer_duration_sec = 1.0;
    q.imu.deskew.enable = true;
    q.lo.pipeline.velocity_update.enable = true;
    Pipeline w(q);
    std::printf("  buffer_duration_sec %.3f, velocity_update.enable %d\n", w.get_params().imu.buffer_duration_sec,
                int(w.get_params().lo.pipeline.velocity_update.enable));
    CHECK(std::fabs(w.get_params().imu.buffer_duration_sec - 1.2) < 1e-6);
    CHECK(!w.get_params().lo.pipeline.velocity_update.enable);
    q.imu.deskew.enable = false;
    Pipeline keep(q);
    CHECK(keep.get_params().lo.pipeline.velocity_update.enable);
}
static void initial_alignment_gate() {
    const float roll = 10.0f * kPi / 180.0f, pitch = -5.0f * kPi / 180.0f, yaw_user = 30.0f * kPi / 180.0f, g = 9.80665f;
    // the specific force of a device at rest with R_world_body = Ry(pitch) Rx(roll): R^T (0, 0, g)
    const V3 force(-std::sin(pitch) * g, std::cos(pitch) * std::sin(roll) * g, std::cos(pitch) * std::cos(roll) * g);
    const V3 gyro(0.002f, -0.001f, 0.003f);
    lo::Parameters params;
    params.imu.enable = true;
    params.pose.initial.matrix() = rigid(yaw_user, 1.0f, 2.0f, 3.0f);
    Pipeline p(params);
    for (int i = 0; i <= 50; ++i) p.add_imu_measurement(sample(9.5 + 0.01 * i, gyro, force));  // 0.5 s < required_duration_sec
    CHECK(p.process(upload(p, g_target), 10.0) == Result::waiting_initial_alignment);
    std::printf("  message: '%s'\n", p.get_error_message().c_str());
    CHECK(p.get_error_message() == "initial_alignment: IMU buffer spans less than required_duration_sec");
    CHECK(max_entry_diff(p.get_odom().matrix(), rigid(yaw_user, 1.0f, 2.0f, 3.0f)) == 0.0f);
    for (int i = 51; i <= 120; ++i) p.add_imu_measurement(sample(9.5 + 0.01 * i, gyro, force));
    CHECK(p.process(upload(p, g_target), 10.7) == Result::first_frame);
    const M4 odom = p.get_odom().matrix();
    print_pose("odom after the alignment", odom);
    // what the estimate gives on the same buffer, with the user's yaw on the left
    const auto res = imu::estimate_initial_alignment(p.get_imu_buffer(), params.imu.preintegration.gravity, params.imu.initial_alignment, imu::IMUBias());
    CHECK(res.success);
    const M3 expect = iso(rigid(yaw_user, 0.0f)).rotation() * res.R_world_imu;
    float worst = 0.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) worst = std::max(worst, std::fabs(odom(i, j) - expect(i, j)));
    std::printf("  roll %.6f (true %.6f), pitch %.6f (true %.6f); |R_odom - Rz(yaw) R_aligned| = %.3g\n", res.roll_rad, roll, res.pitch_rad, pitch, worst);
    CHECK(worst <= 1e-6f);
    CHECK(std::fabs(res.roll_rad - roll) <= 1e-5f && std::fabs(res.pitch_rad - pitch) <= 1e-5f);
    // the tilt itself: the third row of R_odom is the direction of the measured force (a yaw on the left does not touch it)
    for (int j = 0; j < 3; ++j) CHECK(std::fabs(odom(2, j) - force[j] / g) <= 1e-5f);
    CHECK(std::fabs(imu::detail::yaw_from_rotation(iso(odom).rotation()) - yaw_user) <= 0.02f);  // (the minimum rotation's own yaw: about roll * pitch / 2 = 0.008)
    CHECK(odom(0, 3) == 1.0f && odom(1, 3) == 2.0f && odom(2, 3) == 3.0f);
    CHECK(max_entry_diff(p.get_keyframe_poses().front().matrix(), odom) == 0.0f);  // the first keyframe is anchored at the aligned pose
}
static M4 two_identical_frames(lo::MotionPredictionMode mode, bool with_imu, Result* last) {
    lo::Parameters params;
    params.imu.enable = with_imu;
    params.imu.initial_alignment.enable = false;
    params.motion_prediction.mode = mode;
    Pipeline p(params);
    if (with_imu)
        for (int i = 0; i <= 40; ++i) p.add_imu_measurement(sample(0.9 + 0.01 * i, V3(0.0f, 0.0f, 0.0f), V3(0.0f, 0.0f, 9.80665f)));
    const Result first = p.process(upload(p, g_target), 1.0);
    *last = p.process(upload(p, g_target), 1.1);
    if (first != Result::first_frame) *last = Result::error;
    return p.get_odom().matrix();
}
static void motion_prediction_modes() {
    Result r_cv, r_gyro, r_se3;
    const M4 cv = two_identical_frames(lo::MotionPredictionMode::LIDAR_CV, false, &r_cv);
    const M4 gyro = two_identical_frames(lo::MotionPredictionMode::GYRO_LIDAR_CV, true, &r_gyro);
    const M4 se3 = two_identical_frames(lo::MotionPredictionMode::IMU_SE3, true, &r_se3);
    const float bound = std::max(g_hand_spread, 1e-4f);
    std::printf("  results %d %d %d; |GYRO_LIDAR_CV - LIDAR_CV| = %.3g, |IMU_SE3 - LIDAR_CV| = %.3g, bound %.3g; |LIDAR_CV - I| = %.3g\n", int(r_cv),
                int(r_gyro), int(r_se3), max_entry_diff(gyro, cv), max_entry_diff(se3, cv), bound, max_entry_diff(cv, M4::Identity()));
    CHECK(r_cv == Result::success && r_gyro == Result::success && r_se3 == Result::success);
    CHECK(max_entry_diff(gyro, cv) <= bound);
    CHECK(max_entry_diff(se3, cv) <= bound);
    CHECK(max_entry_diff(cv, M4::Identity()) <= 1e-3f);  // the same scan twice: no motion
}

/// target.ply with time stamps spread over 100 ms from `start_sec`
static PointCloudCPU stamped(double start_sec) {
    PointCloudCPU c = g_target;
    c.timestamp_offsets->resize(c.size());
    for (size_t i = 0; i < c.size(); ++i) (*c.timestamp_offsets)[i] = 100.0f * float(i) / float(c.size());
    c.start_time_ms = start_sec * 1e3;
    c.end_time_ms = start_sec * 1e3 + 100.0;
    return c;
}
static void deskew_paths() {
    // the same stamped scan twice: no motion, so both deskews leave the points where they are and the pose is the identity
    {  // IMU deskew of the caller's scan in preprocess (a resting IMU), the velocity update switched off by it
        lo::Parameters params;
        params.imu.enable = true;
        params.imu.initial_alignment.enable = false;
        params.imu.deskew.enable = true;
        params.lo.pipeline.velocity_update.enable = true;
        Pipeline p(params);
        for (int i = 0; i <= 50; ++i) p.add_imu_measurement(sample(0.9 + 0.01 * i, V3(0.0f, 0.0f, 0.0f), V3(0.0f, 0.0f, 9.80665f)));
        const Result r0 = p.process(upload(p, stamped(1.0)), 1.0);
        const Result r1 = p.process(upload(p, stamped(1.1)), 1.1);
        const float d = max_entry_diff(p.get_odom().matrix(), M4::Identity());
        std::printf("  IMU deskew: results %d %d, |pose - I| = %.3g, message '%s'\n", int(r0), int(r1), d, p.get_error_message().c_str());
        CHECK(r0 == Result::first_frame && r1 == Result::success);
        CHECK(d <= 1e-3f);
        CHECK(p.get_preprocessed_point_cloud().size() > 1000 && p.get_preprocessed_point_cloud().has_timestamps());
    }
    {  // the velocity update: deskew-and-realign inside the registration, then the full-resolution cloud in place (a cloud that
       // lives on the device only: shared_vector::device_data_rw must keep its size)
        lo::Parameters params = defaults_without_imu();
        params.lo.pipeline.velocity_update.enable = true;
        params.lo.pipeline.velocity_update.iter = 2;
        Pipeline p(params);
        const Result r0 = p.process(upload(p, stamped(1.0)), 1.0);
        const Result r1 = p.process(upload(p, stamped(1.1)), 1.1);
        const float d = max_entry_diff(p.get_odom().matrix(), M4::Identity());
        std::printf("  velocity update: results %d %d, |pose - I| = %.3g, message '%s'\n", int(r0), int(r1), d, p.get_error_message().c_str());
        CHECK(r0 == Result::first_frame && r1 == Result::success);
        CHECK(d <= 1e-3f);
        CHECK(p.get_preprocessed_point_cloud().size() > 1000 && p.get_preprocessed_point_cloud().has_timestamps());
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <golden dir>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    g_target = PointCloudReader::readFile(dir + "/target.ply");
    g_source = PointCloudReader::readFile(dir + "/source.ply");
    std::ifstream gt(dir + "/T_target_source.txt");
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) gt >> g_T_gt(r, c);
    if (!gt || g_target.size() == 0 || g_source.size() == 0) { std::printf("cannot read the golden files in %s\n", dir.c_str()); return 2; }
    std::printf("target %zu points (intensity %d), source %zu points\n", g_target.size(), int(g_target.has_intensity()), g_source.size());
    RUN(pipeline_is_the_chain);
    RUN(ground_truth);
    RUN(drive_occupancy_grid);
    RUN(drive_voxel_hash_map);
    RUN(result_codes);
    RUN(imu_buffer_rules);
    RUN(initial_alignment_gate);
    RUN(motion_prediction_modes);
    RUN(deskew_paths);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
