// C++ tests of the PolarGrid facade, included through the reference's paths only, modelled on the reference's
// cpp/tests/test_downsampling_filters.cpp:90-136. Built and run by tests/test_gpu_polar_grid.py on a GPU box; exit code 0 = all
// checks passed.
#include <cmath>
#include <cstdio>
#include <stdexcept>

#include <random>

#include "sycl_points/algorithms/common/coordinate_system.hpp"
#include "sycl_points/algorithms/filter/polar_downsampling.hpp"
#include "sycl_points/algorithms/knn/bruteforce.hpp"
#include "sycl_points/algorithms/knn/grid.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"

using namespace sycl_points;
namespace alg = sycl_points::algorithms;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); } while (0)

static sycl_utils::DeviceQueue* Q = nullptr;
static const float kPiF = 3.14159265f;

template <class F>
static bool throws_invalid(F&& f) {
    try { f(); } catch (const std::invalid_argument&) { return true; }
    return false;
}

static void constructor_setters_getters() {
    CHECK(throws_invalid([] { alg::filter::PolarGrid g(*Q, 0.0f, 1.0f, 1.0f); }));
    CHECK(throws_invalid([] { alg::filter::PolarGrid g(*Q, 1.0f, -1.0f, 1.0f); }));
    CHECK(throws_invalid([] { alg::filter::PolarGrid g(*Q, 1.0f, 1.0f, 0.0f); }));
    alg::filter::PolarGrid g(*Q, 0.5f, 0.25f, 0.125f);
    CHECK(g.get_distance_voxel_size() == 0.5f && g.get_elevation_voxel_size() == 0.25f && g.get_azimuth_voxel_size() == 0.125f);
    CHECK(g.get_coordinate_system() == alg::CoordinateSystem::LIDAR && g.get_min_voxel_count() == 1);
    g.set_distance_voxel_size(2.0f);
    g.set_elevation_voxel_size(0.5f);
    g.set_azimuth_voxel_size(0.75f);
    g.set_min_voxel_count(3);
    g.set_coordinate_system(alg::CoordinateSystem::CAMERA);
    CHECK(g.get_distance_voxel_size() == 2.0f && g.get_elevation_voxel_size() == 0.5f && g.get_azimuth_voxel_size() == 0.75f);
    CHECK(g.get_min_voxel_count() == 3 && g.get_coordinate_system() == alg::CoordinateSystem::CAMERA);
    CHECK(throws_invalid([&] { g.set_distance_voxel_size(0.0f); }));
    CHECK(throws_invalid([&] { g.set_elevation_voxel_size(-1.0f); }));
    CHECK(throws_invalid([&] { g.set_azimuth_voxel_size(0.0f); }));
    CHECK(g.get_distance_voxel_size() == 2.0f);
    CHECK(alg::coordinate_system_from_string("lidar") == alg::CoordinateSystem::LIDAR);
    CHECK(alg::coordinate_system_from_string("LiDaR") == alg::CoordinateSystem::LIDAR);
    CHECK(alg::coordinate_system_from_string("CAMERA") == alg::CoordinateSystem::CAMERA);
    CHECK(alg::coordinate_system_from_string("camera") == alg::CoordinateSystem::CAMERA);
    CHECK(throws_invalid([] { alg::coordinate_system_from_string("radar"); }));
    CHECK(throws_invalid([] { alg::coordinate_system_from_string(""); }));
}

// test_downsampling_filters.cpp:90-136: two groups in the distance bins [1, 2) and [2, 3)
static PointCloudCPU known_answer_cloud(bool timestamps) {
    PointCloudCPU c;
    const float xs[5] = {1.10f, 1.40f, 2.10f, 2.30f, 2.40f}, inten[5] = {2.0f, 4.0f, 6.0f, 10.0f, 100.0f};
    for (int i = 0; i < 5; ++i) {
        c.points->push_back(PointType(xs[i], 0.0f, 0.0f, 1.0f));
        c.intensities->push_back(inten[i]);
        if (timestamps) c.timestamp_offsets->push_back(float(2 * i));
    }
    return c;
}

static void known_answer() {
    PointCloudShared cloud(*Q, known_answer_cloud(false)), result(*Q);
    alg::filter::PolarGrid g(*Q, 1.0f, kPiF, kPiF, alg::CoordinateSystem::LIDAR);
    g.set_min_voxel_count(2);
    g.downsampling(cloud, result);
    CHECK(result.size() == 2 && result.has_intensity());
    if (result.size() != 2) return;
    // ascending key order: distance is the least significant field, both voxels share elevation and azimuth
    CHECK(std::fabs((*result.points)[0].x() - 1.25f) < 1e-5f && std::fabs((*result.intensities)[0] - 3.0f) < 1e-5f);
    CHECK(std::fabs((*result.points)[1].x() - 2.2666667f) < 1e-5f && std::fabs((*result.intensities)[1] - 10.0f) < 1e-5f);
    CHECK(!result.has_rgb() && !result.has_timestamps() && !result.has_cov() && !result.has_normal());
    // the PointContainerShared overload: the same means
    PointContainerShared out(*Q);
    g.downsampling(*cloud.points, out);
    CHECK(out.size() == 2 && std::fabs(out[0].x() - 1.25f) < 1e-5f && std::fabs(out[1].x() - 2.2666667f) < 1e-5f);
    // min_voxel_count 3 keeps the second group only; 1 keeps both
    g.set_min_voxel_count(3);
    g.downsampling(cloud, result);
    CHECK(result.size() == 1);
    g.set_min_voxel_count(1);
    g.downsampling(cloud, result);
    CHECK(result.size() == 2);
}

static void in_place_and_timestamps() {
    PointCloudShared cloud(*Q, known_answer_cloud(true));
    cloud.start_time_ms = 1000.0;
    cloud.end_time_ms = 1100.0;
    alg::filter::PolarGrid g(*Q, 1.0f, kPiF, kPiF);
    g.set_min_voxel_count(2);
    g.downsampling(cloud, cloud);  // in place
    CHECK(cloud.size() == 2 && cloud.has_timestamps() && cloud.has_intensity());
    if (cloud.size() == 2) {
        CHECK(std::fabs((*cloud.timestamp_offsets)[0] - 1.0f) < 1e-6f && std::fabs((*cloud.timestamp_offsets)[1] - 6.0f) < 1e-6f);
        CHECK(std::fabs((*cloud.points)[1].x() - 2.2666667f) < 1e-5f);
    }
    CHECK(cloud.start_time_ms == 1000.0 && cloud.end_time_ms == 1100.0);
    // the container overload in place
    PointCloudShared c2(*Q, known_answer_cloud(false));
    g.downsampling(*c2.points, *c2.points);
    CHECK(c2.points->size() == 2 && std::fabs((*c2.points)[0].x() - 1.25f) < 1e-5f);
    // an empty cloud gives an empty result; a cloud of invalid points too
    PointCloudShared empty(*Q), r(*Q);
    g.downsampling(empty, r);
    CHECK(r.size() == 0);
    PointCloudCPU bad;
    bad.points->push_back(PointType(0.0f, 0.0f, 0.0f, 1.0f));        // origin
    bad.points->push_back(PointType(0.0f, 0.0f, 5.0f, 1.0f));        // on the z axis (LIDAR)
    bad.points->push_back(PointType(NAN, 1.0f, 1.0f, 1.0f));
    PointCloudShared badc(*Q, bad);
    g.set_min_voxel_count(1);
    g.downsampling(badc, r);
    CHECK(r.size() == 0);
}

static void camera_frame() {
    // camera frame: a point on the y axis has no horizontal term (invalid); z is forward
    PointCloudCPU c;
    c.points->push_back(PointType(0.0f, 3.0f, 0.0f, 1.0f));
    c.points->push_back(PointType(0.0f, 0.0f, 1.2f, 1.0f));
    c.points->push_back(PointType(0.0f, 0.0f, 1.6f, 1.0f));
    PointCloudShared cloud(*Q, c), result(*Q);
    alg::filter::PolarGrid g(*Q, 1.0f, kPiF, kPiF, alg::coordinate_system_from_string("camera"));
    g.downsampling(cloud, result);
    CHECK(result.size() == 1);
    if (result.size() == 1) CHECK(std::fabs((*result.points)[0].z() - 1.4f) < 1e-6f);
}

static void knn_on_the_output() {
    // a structure built on PolarGrid's output finds what brute force finds (no Cartesian bounds are assumed for it)
    std::mt19937 gen(7);
    std::uniform_real_distribution<float> az(-kPiF, kPiF), el(-0.4f, 0.3f), rr(1.0f, 40.0f);
    PointCloudCPU c;
    for (int i = 0; i < 20000; ++i) {
        const float a = az(gen), e = el(gen), r = rr(gen);
        c.points->push_back(PointType(r * std::cos(e) * std::cos(a), r * std::cos(e) * std::sin(a), r * std::sin(e), 1.0f));
    }
    PointCloudShared cloud(*Q, c), out(*Q);
    alg::filter::PolarGrid g(*Q, 0.5f, 0.02f, 0.02f);
    g.downsampling(cloud, out);
    CHECK(out.size() > 1000 && out.size() < 20000);
    PointCloudCPU qc;
    for (int i = 0; i < 300; ++i) qc.points->push_back(PointType(rr(gen) * 0.5f, rr(gen) * 0.5f - 10.0f, el(gen), 1.0f));
    PointCloudShared query(*Q, qc);
    auto grid = alg::knn::GridKNN::build(*Q, out, 1.0f);
    auto tree = alg::knn::KDTree::build(*Q, out);
    for (size_t k : {1, 5, 10}) {
        auto bf = alg::knn::knn_search_bruteforce(*Q, query, out, k);
        auto gr = grid->knn_search(query, k);
        auto kd = tree->knn_search(query, k);
        bool same = true;
        for (size_t i = 0; i < 300 * k; ++i)
            same = same && (*gr.indices)[i] == (*bf.indices)[i] && (*gr.distances)[i] == (*bf.distances)[i] &&
                   (*kd.indices)[i] == (*bf.indices)[i] && (*kd.distances)[i] == (*bf.distances)[i];
        CHECK(same);
    }
}

int main() {
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(constructor_setters_getters);
    RUN(known_answer);
    RUN(in_place_and_timestamps);
    RUN(camera_frame);
    RUN(knn_on_the_output);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
