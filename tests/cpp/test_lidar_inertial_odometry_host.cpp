// Host-only C++ checks of the LiDAR-inertial odometry pipeline's facade: no device is touched, so the program runs in the CPU suite
// (tests/test_lidar_inertial_odometry_cpu.py builds it with tests/cpp/Makefile's flags).
//   the two forwarding headers at the reference's paths give the reference's types under the reference's names (nothing is
//   included before them here; the pytest file also compiles each as a translation unit of its own)
//   every default of the LIO parameter block (lidar_inertial_odometry_params.hpp:15-57)
//   the ResultType values (lidar_inertial_odometry.hpp:60-68)
// Exit code 0 = all checks passed.
#include "sycl_points/pipeline/lidar_inertial_odometry_params.hpp"

#include "sycl_points/pipeline/lidar_inertial_odometry.hpp"

#include <cstdio>
#include <type_traits>

namespace lio = sycl_points::pipeline::lidar_inertial_odometry;
namespace od = sycl_points::pipeline::odometry;
namespace reg = sycl_points::algorithms::registration;
using Pipeline = lio::LidarInertialOdometryPipeline;
using Result = Pipeline::ResultType;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); } while (0)

static void types_at_the_reference_names() {
    static_assert(std::is_base_of_v<od::CommonParameters, lio::Parameters>);
    static_assert(std::is_same_v<Pipeline::Ptr, std::shared_ptr<Pipeline>>);
    static_assert(std::is_same_v<Pipeline::ConstPtr, std::shared_ptr<const Pipeline>>);
    static_assert(std::is_same_v<std::underlying_type_t<Result>, std::int8_t>);
    static_assert(std::is_same_v<decltype(lio::Parameters::LIO::registration), sycl_points::algorithms::lio::LIORegistrationParams>);
    static_assert(std::is_constructible_v<Pipeline, const lio::Parameters&>);
    static_assert(!std::is_convertible_v<const lio::Parameters&, Pipeline>);  // explicit, as the reference's
    CHECK(true);
}

static void lio_block_defaults() {
    const lio::Parameters p;
    CHECK(p.lio.preintegration_reset.fd_velocity_sigma == 0.1f);
    CHECK(p.lio.preintegration_reset.icp_rotation_sigma == 0.01f);
    CHECK(!p.lio.bias_estimation.freeze_on_low_excitation);
    CHECK(p.lio.bias_estimation.gyro_excitation_threshold == 0.03f);
    CHECK(p.lio.bias_estimation.accel_excitation_threshold == 0.3f);
    CHECK(p.lio.bias_estimation.max_accel_bias == 0.0f);
    CHECK(p.lio.bias_estimation.max_gyro_bias == 0.0f);
    // registration: an algorithms::lio::LIORegistrationParams with its own defaults (lio_registration_params.hpp:11-49)
    CHECK(p.lio.registration.total_iterations == 10 && p.lio.registration.invalid_regularization_factor == 1e4f);
    CHECK(!p.lio.registration.robust.auto_scale && p.lio.registration.robust.init_scale == 10.0f && p.lio.registration.robust.min_scale == 0.5f &&
          p.lio.registration.robust.auto_scaling_iter == 4);
    CHECK(p.lio.registration.directional_icp_weighting.enable);
    // the common block is the LiDAR pipeline's: the IMU is off in the struct (the pipeline's constructor forces it on)
    CHECK(!p.imu.enable && p.imu.buffer_duration_sec == 1.0 && p.imu.initial_alignment.enable);
    CHECK(p.registration.min_num_points == 100 && p.registration.factor.reg_type == reg::RegType::GICP);
    CHECK(p.registration_sampling.enable && p.registration_sampling.num == 1000 && p.submap.point_random_sampling_num == 512);
}

static void result_type_values() {
    CHECK(int(Result::success) == 0);
    CHECK(int(Result::first_frame) == 1);
    CHECK(int(Result::waiting_initial_alignment) == 2);
    CHECK(int(Result::imu_only) == 3);
    CHECK(int(Result::error) == 100);
    CHECK(int(Result::old_timestamp) == 101);
    CHECK(int(Result::small_number_of_points) == 102);
}

int main() {
    RUN(types_at_the_reference_names);
    RUN(lio_block_defaults);
    RUN(result_type_values);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
