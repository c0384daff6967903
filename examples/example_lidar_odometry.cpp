// The per-frame odometry loop on the facade: the scans given on the command line go through
// pipeline::lidar_odometry::LiDAROdometryPipeline::process one after the other, 0.1 s apart, with the reference's default
// parameters (IMU off); the pose and the four stage times are printed after every scan.
// usage: example_lidar_odometry <first.ply> <second.ply> [more.ply ...]
#include <cstdio>
#include <string>

#include "sycl_points/io/point_cloud_reader.hpp"
#include "sycl_points/pipeline/lidar_odometry.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s first.ply second.ply [more.ply ...]\n", argv[0]); return 2; }
    namespace lo = sycl_points::pipeline::lidar_odometry;
    lo::Parameters params;
    params.imu.enable = false;
    params.motion_prediction.mode = lo::MotionPredictionMode::LIDAR_CV;
    lo::LiDAROdometryPipeline pipeline(params);
    pipeline.get_device_queue()->print_device_info();

    using Result = lo::LiDAROdometryPipeline::ResultType;
    for (int i = 1; i < argc; ++i) {
        const auto cpu = sycl_points::PointCloudReader::readFile(argv[i]);
        const auto scan = std::make_shared<sycl_points::PointCloudShared>(*pipeline.get_device_queue(), cpu);
        const double timestamp = 1.0 + 0.1 * (i - 1);  // (a stamp of 0.0 reads as "no frame yet", pipeline/lidar_odometry.hpp:131)
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
            std::printf("inliers %u of %zu, submap %zu points\n", pipeline.get_registration_result().inlier,
                        pipeline.get_registration_input_point_cloud()->size(), pipeline.get_submap_point_cloud().size());
    }
    const sycl_points::TransformMatrix T = pipeline.get_odom().matrix();
    std::printf("RESULT");
    for (int i = 0; i < 16; ++i) std::printf(" %.9g", T.data()[i]);
    std::printf("\n");
    return 0;
}
