// C++ tests of the OccupancyGridMap facade, included through the reference's path only: the reference's own cases
// (cpp/tests/test_occupancy_grid_map.cpp:90-523, restated with their tolerances, without the extract_visible_points ones) and one
// carving case with its exact probabilities. Built and run by tests/test_gpu_occupancy_grid.py on a GPU box; exit code 0 = all passed.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "sycl_points/algorithms/mapping/occupancy_grid_map.hpp"

using namespace sycl_points;
using OGM = sycl_points::algorithms::mapping::OccupancyGridMap;
using V3 = Eigen::Vector3f;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); } while (0)

static sycl_utils::DeviceQueue* Q = nullptr;
static const Eigen::Isometry3f I = Eigen::Isometry3f::Identity();

static PointCloudCPU make(std::initializer_list<std::array<float, 3>> pts) {
    PointCloudCPU c;
    for (const auto& p : pts) c.points->emplace_back(p[0], p[1], p[2], 1.0f);
    return c;
}
static Covariance cov(float xx, float xy, float xz, float yy, float yz, float zz) {
    Covariance m = Covariance::Zero();
    m(0, 0) = xx; m(0, 1) = m(1, 0) = xy; m(0, 2) = m(2, 0) = xz; m(1, 1) = yy; m(1, 2) = m(2, 1) = yz; m(2, 2) = zz;
    return m;
}
// exp((log C0 + log C1) / 2) of aggregates_attributes' two covariances, evaluated in float64 (numpy.linalg.eigh), upper triangle
static const double kMeanCov[3][3] = {{1.732085976156, 0.348213415492, 0.525275760137}, {0.348213415492, 2.827654500891, 0.564482139205}, {0.525275760137, 0.564482139205, 3.869196084465}};
static float logistic(float l) { return 1.0f / (1.0f + std::exp(-l)); }

static void constructor_and_setters_validate() {  // :90-95, and the setters' std::invalid_argument (:73-121)
    for (const float bad : {0.0f, -0.1f}) {
        bool threw = false;
        try { OGM m(*Q, bad); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw);
    }
    OGM m(*Q, 0.25f);
    CHECK(m.voxel_size() == 0.25f);
    int thrown = 0;
    try { m.set_voxel_size(0.0f); } catch (const std::invalid_argument&) { ++thrown; }
    try { m.set_log_odds_limits(1.0f, -1.0f); } catch (const std::invalid_argument&) { ++thrown; }
    try { m.set_occupancy_threshold(0.0f); } catch (const std::invalid_argument&) { ++thrown; }
    try { m.set_occupancy_threshold(1.0f); } catch (const std::invalid_argument&) { ++thrown; }
    CHECK(thrown == 4);
    m.set_log_odds_limits(-2.0f, 3.5f);
    m.set_occupancy_threshold(0.7f);
    m.set_stale_frame_threshold(7);
}

static void integrates_points_and_skips_far_voxels() {  // :97-135, 141-165
    {
        OGM map(*Q, 0.2f);
        map.add_point_cloud(PointCloudShared(*Q, make({{0.05f, 0.05f, 0.0f}, {0.07f, 0.05f, 0.0f}, {0.35f, 0.05f, 0.0f}})), I);
        PointCloudShared result(*Q);
        map.extract_occupied_points(result, I, 1.0f);
        CHECK(result.size() == 2);
        if (result.size() == 2) {
            std::vector<PointType> v{(*result.points)[0], (*result.points)[1]};
            if (v[0].x() > v[1].x()) std::swap(v[0], v[1]);
            CHECK(std::fabs(v[0].x() - 0.06f) <= 1e-5f && std::fabs(v[0].y() - 0.05f) <= 1e-5f && std::fabs(v[0].z()) <= 1e-5f);
            CHECK(std::fabs(v[1].x() - 0.35f) <= 1e-5f && std::fabs(v[1].y() - 0.05f) <= 1e-5f && std::fabs(v[1].z()) <= 1e-5f);
            CHECK(v[0].w() == 1.0f && v[1].w() == 1.0f);
        }
        CHECK(!result.has_cov() && !result.has_rgb() && !result.has_intensity());
    }
    {
        OGM map(*Q, 0.2f);
        map.add_point_cloud(PointCloudShared(*Q, make({{0.0f, 0.0f, 0.0f}, {5.0f, 0.0f, 0.0f}})), I);
        PointCloudShared result(*Q);
        map.extract_occupied_points(result, I, 1.0f);
        CHECK(result.size() == 1);
        if (result.size() == 1) CHECK(std::fabs((*result.points)[0].x()) <= 1e-5f);
    }
    {  // early returns (:130-132, 176-178, 418-420)
        OGM map(*Q, 0.2f);
        PointCloudShared empty(*Q), result(*Q);
        map.add_point_cloud(empty, I);
        map.extract_occupied_points(result, I);
        CHECK(result.size() == 0 && map.compute_overlap_ratio(empty, I) == 0.0f);
        CHECK(map.compute_overlap_ratio(PointCloudShared(*Q, make({{0.f, 0.f, 0.f}})), I) == 0.0f);
    }
}

static void overlap_ratio() {  // :167-202
    OGM map(*Q, 0.5f);
    const PointCloudShared map_cloud(*Q, make({{0.1f, 0.1f, 0.0f}, {1.1f, 0.0f, 0.0f}}));
    map.add_point_cloud(map_cloud, I);
    const PointCloudShared query(*Q, make({{-0.9f, 0.1f, 0.0f}, {0.1f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}}));
    Eigen::Isometry3f pose = Eigen::Isometry3f::Identity();
    pose.matrix()(0, 3) = 1.0f;
    CHECK(std::fabs(map.compute_overlap_ratio(query, pose) - 2.0f / 3.0f) <= 1e-5f);
    map.set_occupancy_threshold(0.8f);
    CHECK(std::fabs(map.compute_overlap_ratio(query, pose)) <= 1e-5f);
    map.add_point_cloud(map_cloud, I);
    CHECK(std::fabs(map.compute_overlap_ratio(query, pose) - 2.0f / 3.0f) <= 1e-5f);
}

static void aggregates_attributes() {  // :208-247, 253-301, 349-366
    const std::vector<Covariance> covs{cov(1.0f, 0.2f, 0.3f, 2.0f, 0.4f, 3.0f), cov(3.0f, 0.6f, 0.9f, 4.0f, 0.8f, 5.0f)};
    for (const bool with_cov : {false, true}) {
        OGM map(*Q, 0.1f);
        PointCloudCPU c = make({{0.f, 0.f, 0.f}, {0.05f, 0.f, 0.f}});
        c.rgb->emplace_back(0.0f, 0.2f, 0.4f, 1.0f);
        c.rgb->emplace_back(0.2f, 0.4f, 0.6f, 1.0f);
        *c.intensities = {10.0f, 30.0f};
        if (with_cov) for (const auto& m : covs) c.covs->push_back(m);
        map.add_point_cloud(PointCloudShared(*Q, c), I);
        PointCloudShared result(*Q);
        map.extract_occupied_points(result, I, 1.0f);
        CHECK(result.size() == 1 && result.has_rgb() && result.has_intensity() && result.has_cov() == with_cov);
        if (result.size() != 1 || !result.has_rgb() || !result.has_intensity() || result.has_cov() != with_cov) continue;
        const PointType p = (*result.points)[0];
        CHECK(std::fabs(p.x() - 0.025f) <= 1e-5f && std::fabs(p.y()) <= 1e-5f && std::fabs(p.z()) <= 1e-5f);
        const RGBType col = (*result.rgb)[0];
        CHECK(std::fabs(col.x() - 0.1f) <= 1e-5f && std::fabs(col.y() - 0.3f) <= 1e-5f && std::fabs(col.z() - 0.5f) <= 1e-5f &&
              std::fabs(col.w() - 1.0f) <= 1e-5f);
        CHECK(std::fabs((*result.intensities)[0] - 20.0f) <= 1e-5f);
        if (with_cov) {
            const Covariance got = (*result.covs)[0];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) CHECK(std::fabs(double(got(i, j)) - kMeanCov[i][j]) <= 1e-5);
            for (int k = 0; k < 4; ++k) CHECK(std::fabs(got(3, k)) <= 1e-5f && std::fabs(got(k, 3)) <= 1e-5f);
        }
    }
}

static void rotates_covariances_into_map_frame() {  // :303-347
    const std::vector<Covariance> covs{cov(1.0f, 0.0f, 0.0f, 4.0f, 0.0f, 9.0f), cov(9.0f, 0.0f, 0.0f, 16.0f, 0.0f, 25.0f)};
    OGM map(*Q, 0.5f);
    PointCloudCPU c = make({{0.f, 0.f, 0.f}, {0.1f, 0.f, 0.f}});
    for (const auto& m : covs) c.covs->push_back(m);
    Eigen::Isometry3f pose = Eigen::Isometry3f::Identity();
    const float th = 3.14159265358979323846f / 2.0f;  // about z
    pose.matrix()(0, 0) = std::cos(th); pose.matrix()(0, 1) = -std::sin(th);
    pose.matrix()(1, 0) = std::sin(th); pose.matrix()(1, 1) = std::cos(th);
    pose.matrix()(0, 3) = 1.0f;
    map.add_point_cloud(PointCloudShared(*Q, c), pose);
    PointCloudShared result(*Q);
    map.extract_occupied_points(result, pose, 1.0f);
    CHECK(result.size() == 1 && result.has_cov());
    if (result.size() == 1 && result.has_cov()) {
        // the log-Euclidean mean of two diagonal matrices is the geometric mean of their entries, diag(3, 8, 15); turned by a
        // quarter about z: diag(8, 3, 15)
        const float want[3][3] = {{8.0f, 0.0f, 0.0f}, {0.0f, 3.0f, 0.0f}, {0.0f, 0.0f, 15.0f}};
        const Covariance got = (*result.covs)[0];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) CHECK(std::fabs(got(i, j) - want[i][j]) <= 1e-4f);
    }
}

static void free_space_along_a_ray() {  // :368-392, 394-412, and the values behind their inequalities
    for (const bool carving : {true, false}) {
        OGM map(*Q, 0.1f);
        map.set_log_odds_hit(0.9f);
        map.set_log_odds_miss(-0.6f);
        map.set_free_space_updates_enabled(carving);
        map.add_point_cloud(PointCloudShared(*Q, make({{0.45f, 0.0f, 0.0f}})), I);
        const float free_p = map.voxel_probability(V3(0.05f, 0.0f, 0.0f));
        CHECK(carving ? free_p < 0.5f : std::fabs(free_p - 0.5f) <= 1e-5f);
        CHECK(map.voxel_probability(V3(0.45f, 0.0f, 0.0f)) > 0.5f);
        CHECK(std::fabs(map.voxel_probability(V3(0.45f, 0.0f, 0.0f)) - logistic(0.9f)) <= 1e-5f);
        for (const float x : {0.05f, 0.15f, 0.25f, 0.35f})  // the origin's cell and the three between: one miss each
            CHECK(std::fabs(map.voxel_probability(V3(x, 0.0f, 0.0f)) - (carving ? logistic(-0.6f) : 0.5f)) <= 1e-5f);
        CHECK(std::fabs(map.voxel_probability(V3(0.55f, 0.0f, 0.0f)) - 0.5f) <= 1e-5f);  // beyond the hit: untouched
    }
}

static void carving_a_diagonal_ray() {  // the facade's one carving case beyond the reference's: a ray that changes all three cells
    OGM map(*Q, 0.5f);
    map.set_log_odds_hit(1.0f);
    map.set_log_odds_miss(-0.5f);
    Eigen::Isometry3f pose = Eigen::Isometry3f::Identity();
    pose.matrix()(0, 3) = 0.2f; pose.matrix()(1, 3) = 0.3f; pose.matrix()(2, 3) = 0.1f;
    map.add_point_cloud(PointCloudShared(*Q, make({{1.0f, 0.6f, 0.5f}})), pose);  // map frame: (1.2, 0.9, 0.6), cell (2, 1, 1)
    // from (0.4, 0.6, 0.2) cells to (2.4, 1.8, 1.2): t_y = 1/3 -> t_x = 0.3 first: x at t = 0.3, y at 0.333, z at 0.8, x at 0.8
    // (tie: x first)
    const std::array<std::array<float, 3>, 4> missed{{{0.2f, 0.3f, 0.1f}, {0.7f, 0.3f, 0.1f}, {0.7f, 0.7f, 0.1f}, {1.2f, 0.7f, 0.1f}}};
    for (const auto& c : missed) CHECK(std::fabs(map.voxel_probability(V3(c[0], c[1], c[2])) - logistic(-0.5f)) <= 1e-5f);
    CHECK(std::fabs(map.voxel_probability(V3(1.2f, 0.9f, 0.6f)) - logistic(1.0f)) <= 1e-5f);
    CHECK(std::fabs(map.voxel_probability(V3(0.7f, 0.7f, 0.6f)) - 0.5f) <= 1e-5f);
    PointCloudShared result(*Q);
    map.extract_occupied_points(result, pose, 5.0f);
    CHECK(result.size() == 1);
}

static void repeated_observations_and_pruning() {  // :421-456, 458-489, 491-528
    {
        OGM map(*Q, 0.1f);
        map.set_log_odds_hit(1.0f);
        map.set_log_odds_miss(-0.5f);
        map.add_point_cloud(PointCloudShared(*Q, make({{0.0f, 0.0f, 0.0f}, {0.2f, 0.0f, 0.0f}})), I);
        map.add_point_cloud(PointCloudShared(*Q, make({{0.0f, 0.0f, 0.0f}})), I);
        PointCloudShared result(*Q);
        map.extract_occupied_points(result, I, 1.0f);
        CHECK(result.size() == 2);
        if (result.size() == 2) {
            std::vector<PointType> v{(*result.points)[0], (*result.points)[1]};
            if (v[0].x() > v[1].x()) std::swap(v[0], v[1]);
            CHECK(map.voxel_probability(V3(v[1].x(), v[1].y(), v[1].z())) < map.voxel_probability(V3(v[0].x(), v[0].y(), v[0].z())));
        }
    }
    {
        OGM map(*Q, 0.1f);
        map.set_log_odds_hit(1.0f);
        map.set_log_odds_miss(-0.5f);
        map.add_point_cloud(PointCloudShared(*Q, make({{0.0f, 0.0f, 0.0f}, {0.2f, 0.0f, 0.0f}})), I);
        const float base = map.voxel_probability(V3(0.2f, 0.0f, 0.0f));
        map.set_voxel_pruning_enabled(false);
        map.add_point_cloud(PointCloudShared(*Q, make({{0.0f, 0.0f, 0.0f}})), I);
        CHECK(std::fabs(map.voxel_probability(V3(0.2f, 0.0f, 0.0f)) - base) <= 1e-5f);
    }
    {
        OGM map(*Q, 0.1f);
        map.set_log_odds_hit(1.0f);
        map.set_log_odds_miss(-0.5f);
        map.set_free_space_updates_enabled(false);
        map.set_voxel_pruning_enabled(true);
        map.set_stale_frame_threshold(100U);
        map.add_point_cloud(PointCloudShared(*Q, make({{0.0f, 0.0f, 0.0f}})), I);
        const PointCloudShared filler(*Q, make({{1.0f, 0.0f, 0.0f}}));
        for (uint32_t i = 0; i <= 100U; ++i) map.add_point_cloud(filler, I);
        CHECK(std::fabs(map.voxel_probability(V3(0.0f, 0.0f, 0.0f)) - 0.5f) <= 1e-5f);
        CHECK(map.voxel_probability(V3(1.0f, 0.0f, 0.0f)) > 0.5f);
        map.clear();
        CHECK(std::fabs(map.voxel_probability(V3(1.0f, 0.0f, 0.0f)) - 0.5f) <= 1e-5f);
    }
}

int main() {
    sycl_utils::DeviceQueue queue;
    Q = &queue;
    RUN(constructor_and_setters_validate);
    RUN(integrates_points_and_skips_far_voxels);
    RUN(overlap_ratio);
    RUN(aggregates_attributes);
    RUN(rotates_covariances_into_map_frame);
    RUN(free_space_along_a_ray);
    RUN(carving_a_diagonal_ray);
    RUN(repeated_observations_and_pruning);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
