// The per-frame LiDAR-inertial odometry loop on the facade: the scans given on the command line go through
// pipeline::lidar_inertial_odometry::LidarInertialOdometryPipeline::process one after the other, 0.1 s apart, with a synthesised
// IMU at rest (200 Hz, specific force (0, 0, g), no rotation) and the noise densities of the reference's
// config/lidar_inertial_odometry.yaml; the pose and the four stage times are printed after every scan, the final state at the end.
// usage: example_lidar_inertial_odometry <first.ply> <second.ply> [more.ply ...]
#include <cstdio>
#include <string>

#include "sycl_points/io/point_cloud_reader.hpp"
#include "sycl_points/pipeline/lidar_inertial_odometry.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s first.ply second.ply [more.ply ...]\n", argv[0]); return 2; }
    namespace lio = sycl_points::pipeline::lidar_inertial_odometry;
    lio::Parameters params;
    params.imu.initial_alignment.enable = false;  // (it would wait for one second of stationary samples before the first scan)
    params.imu.preintegration.gyro_noise_density = 1e-2f;
    params.imu.preintegration.accel_noise_density = 1e-3f;
    params.imu.preintegration.gyro_bias_rw_density = 1e-5f;
    params.imu.preintegration.accel_bias_rw_density = 1e-4f;
    lio::LidarInertialOdometryPipeline pipeline(params);
    pipeline.get_device_queue()->print_device_info();

    using Result = lio::LidarInertialOdometryPipeline::ResultType;
    constexpr double imu_period = 0.005;
    int imu_tick = 180;  // 0.9 s: the buffer starts before the first scan
    for (int i = 1; i < argc; ++i) {
        const auto cpu = sycl_points::PointCloudReader::readFile(argv[i]);
        const auto scan = std::make_shared<sycl_points::PointCloudShared>(*pipeline.get_device_queue(), cpu);
        // (a stamp of 0.0 reads as "no frame yet", pipeline/lidar_inertial_odometry.hpp:146)
        const double timestamp = (200 + 20 * (i - 1)) * imu_period;
        for (; imu_tick * imu_period <= timestamp + 2 * imu_period; ++imu_tick) {  // what an IMU driver has delivered by then
            sycl_points::imu::IMUMeasurement m;
            m.timestamp = imu_tick * imu_period;
            m.accel = Eigen::Vector3f(0.0f, 0.0f, 9.80665f);
            pipeline.add_imu_measurement(m);
        }
        const Result result = pipeline.process(scan, timestamp);
        std::printf("scan %d: %s, %zu points -> %zu preprocessed, result %d%s%s\n", i, argv[i], cpu.size(),
                    pipeline.get_preprocessed_point_cloud().size(), int(result), pipeline.get_error_message().empty() ? "" : ": ",
                    pipeline.get_error_message().c_str());
        if (result != Result::success && result != Result::first_frame) return 1;
        const sycl_points::TransformMatrix T = pipeline.get_odom().matrix();
        std::printf("T_odom_lidar =\n");
        for (int r = 0; r < 4; ++r) std::printf("  % .6f % .6f % .6f % .6f\n", T(r, 0), T(r, 1), T(r, 2), T(r, 3));
        for (const auto& [stage, us] : pipeline.get_current_processing_time()) std::printf("%28s: %10.2f us\n", stage.c_str(), us);
        if (result == Result::success)
            std::printf("inliers %u, iterations %zu, submap %zu points\n", pipeline.get_registration_result().inlier,
                        pipeline.get_registration_result().iterations, pipeline.get_submap_point_cloud().size());
    }
    const sycl_points::TransformMatrix T = pipeline.get_odom().matrix();
    std::printf("RESULT");
    for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
    std::printf("\n");
    const sycl_points::imu::State& x = pipeline.get_lio_state();
    std::printf("STATE velocity % .6f % .6f % .6f accel_bias % .6g % .6g % .6g gyro_bias % .6g % .6g % .6g\n", x.velocity[0], x.velocity[1],
                x.velocity[2], x.accel_bias[0], x.accel_bias[1], x.accel_bias[2], x.gyro_bias[0], x.gyro_bias[1], x.gyro_bias[2]);
    return 0;
}
