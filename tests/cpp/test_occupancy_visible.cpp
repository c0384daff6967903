// C++ tests of OccupancyGridMap::extract_visible_points through the facade, included through the reference's path only: the
// reference's three cases (cpp/tests/test_occupancy_grid_map.cpp:530-627, with their tolerance) and the wall of
// tests/test_occupancy_visible_cpu.py, whose counts follow from its geometry. Built and run by tests/test_gpu_occupancy_visible.py on
// a GPU box; exit code 0 = all passed.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <vector>

#include "sycl_points/algorithms/mapping/occupancy_grid_map.hpp"

using namespace sycl_points;
using OGM = sycl_points::algorithms::mapping::OccupancyGridMap;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); } while (0)

static sycl_utils::DeviceQueue* Q = nullptr;
static const Eigen::Isometry3f I = Eigen::Isometry3f::Identity();
constexpr float kPi = 3.14159265358979323846f;

static PointCloudCPU make(const std::vector<std::array<float, 3>>& pts) {
    PointCloudCPU c;
    for (const auto& p : pts) c.points->emplace_back(p[0], p[1], p[2], 1.0f);
    return c;
}
static bool near(const PointType& p, float x, float y, float z) {
    return std::fabs(p.x() - x) <= 1e-5f && std::fabs(p.y() - y) <= 1e-5f && std::fabs(p.z() - z) <= 1e-5f;
}

static void filters_by_view_frustum() {  // :530-561
    OGM map(*Q, 0.1f);
    map.add_point_cloud(PointCloudShared(*Q, make({{1.0f, 0.0f, 0.0f}, {0.5f, 0.5f, 0.0f}, {-1.0f, 0.0f, 0.0f}})), I);
    const float fov = kPi / 6.0f;
    PointCloudShared result(*Q);
    map.extract_visible_points(result, I, 5.0f, fov, fov);
    CHECK(result.size() == 1);
    if (result.size() == 1) CHECK(near((*result.points)[0], 1.0f, 0.0f, 0.0f) && (*result.points)[0].w() == 1.0f);
    CHECK(!result.has_cov() && !result.has_rgb() && !result.has_intensity());
}

static void includes_backward_when_fov_is_wide() {  // :563-595
    OGM map(*Q, 0.1f);
    map.add_point_cloud(PointCloudShared(*Q, make({{1.0f, 0.0f, 0.0f}, {-1.0f, 0.0f, 0.0f}})), I);
    PointCloudShared result(*Q);
    map.extract_visible_points(result, I, 5.0f, kPi, kPi);
    CHECK(result.size() == 2);
    if (result.size() == 2) {
        std::vector<float> x{(*result.points)[0].x(), (*result.points)[1].x()};
        std::sort(x.begin(), x.end());
        CHECK(std::fabs(x[0] + 1.0f) <= 1e-5f && std::fabs(x[1] - 1.0f) <= 1e-5f);
    }
}

static void respects_occlusion() {  // :597-627
    OGM map(*Q, 0.2f);
    map.add_point_cloud(PointCloudShared(*Q, make({{0.8f, 0.0f, 0.0f}, {1.6f, 0.0f, 0.0f}})), I);
    PointCloudShared result(*Q);
    map.extract_visible_points(result, I, 5.0f, kPi / 2.0f, kPi / 2.0f);
    CHECK(result.size() == 1);
    if (result.size() == 1) CHECK(near((*result.points)[0], 0.8f, 0.0f, 0.0f));
}

// voxel 0.5: a 21 x 21 plane of cell centres at x-cell 4, an 11 x 11 plane at x-cell 8, seen from beside the origin through
// pi/2 x pi/2. Without carving the front plane hides the back plane: 72 voxels, all at x = 2.25. With carving the frame's own rays
// to the back plane open the front plane: 467 voxels stay occupied, 139 are visible, from both planes.
static void a_wall_hides_what_is_behind_it() {
    std::vector<std::array<float, 3>> pts;
    for (int j = -10; j <= 10; ++j)
        for (int k = -10; k <= 10; ++k) pts.push_back({2.25f, (j + 0.5f) * 0.5f, (k + 0.5f) * 0.5f});
    for (int j = -5; j <= 5; ++j)
        for (int k = -5; k <= 5; ++k) pts.push_back({4.25f, (j + 0.5f) * 0.5f, (k + 0.5f) * 0.5f});
    Eigen::Isometry3f sensor = Eigen::Isometry3f::Identity();
    sensor.matrix()(0, 3) = 0.137f; sensor.matrix()(1, 3) = -0.211f; sensor.matrix()(2, 3) = 0.123f;
    for (const bool carving : {false, true}) {
        OGM map(*Q, 0.5f);
        map.set_free_space_updates_enabled(carving);
        map.add_point_cloud(PointCloudShared(*Q, make(pts)), I);
        PointCloudShared occupied(*Q), result(*Q);
        map.extract_occupied_points(occupied, sensor, 100.0f);
        map.extract_visible_points(result, sensor, 100.0f, kPi / 2.0f, kPi / 2.0f);
        std::printf("  carving %d: %zu occupied, %zu visible\n", (int)carving, occupied.size(), result.size());
        CHECK(occupied.size() == (carving ? 467u : 562u));
        CHECK(result.size() == (carving ? 139u : 72u));
        size_t front = 0, back = 0;
        for (size_t i = 0; i < result.size(); ++i) {
            front += (*result.points)[i].x() == 2.25f;
            back += (*result.points)[i].x() == 4.25f;
        }
        CHECK(front + back == result.size() && front > 0 && (carving ? back > 0 : back == 0));
    }
}

static void empty_map_clears_the_result() {
    OGM map(*Q, 0.5f);
    PointCloudShared result(*Q, make({{1.0f, 2.0f, 3.0f}}));
    map.extract_visible_points(result, I, 5.0f, 1.0f, 1.0f);
    CHECK(result.size() == 0 && !result.has_cov() && !result.has_rgb() && !result.has_intensity());
}

int main() {
    sycl_utils::DeviceQueue queue;
    Q = &queue;
    RUN(filters_by_view_frustum);
    RUN(includes_backward_when_fov_is_wide);
    RUN(respects_occlusion);
    RUN(a_wall_hides_what_is_behind_it);
    RUN(empty_map_clears_the_result);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
