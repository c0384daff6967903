// C++ test of Registration::align(source, VoxelHashMap&) — voxelised GICP — through the reference's include paths. Built and run
// by tests/test_gpu_voxel_registration.py on a GPU box: test_voxel_registration <scene file>; exit code 0 = all checks passed.
// The scene file (written by that test): int32 n_target, n_source | target points (4 floats each) | target covariances (16 floats,
// column-major) | source points | source covariances. The target is one point per 0.5 m voxel, so the map this program builds
// holds the very sums the map of the Python test holds, whatever the order of the accumulation.
//   1. GN with 1 cell and LM with 7 cells from the identity: the poses are printed as bit patterns ("T <name> <16 hex words>",
//      column-major) and compared bit for bit with Registration.align_voxel_map by the Python test
//   2. the map changes under a Registration that has aligned against it (a second frame): align() refreshes the rows by itself
//   3. an empty source returns the initial guess; POINT_TO_PLANE, the rotation constraint and set_voxel_neighbors(5) throw
//      std::invalid_argument; GICP without source covariances throws std::runtime_error
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sycl_points/algorithms/mapping/voxel_hash_map.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"

using namespace sycl_points;
namespace alg = sycl_points::algorithms;
namespace reg = sycl_points::algorithms::registration;
using M4 = Eigen::Matrix4f;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static PointCloudCPU read_cloud(std::ifstream& f, int n) {
    PointCloudCPU c;
    c.points->resize(n);
    c.covs->resize(n);
    f.read(reinterpret_cast<char*>(c.points->data()), sizeof(float) * 4 * n);
    f.read(reinterpret_cast<char*>(c.covs->data()), sizeof(float) * 16 * n);
    return c;
}
static void print_pose(const char* name, const M4& T) {
    std::printf("T %s", name);
    for (int i = 0; i < 16; ++i) {
        uint32_t w;
        std::memcpy(&w, T.data() + i, sizeof w);
        std::printf(" %08x", w);
    }
    std::printf("\n");
}
static reg::RegistrationParams params(reg::OptimizationMethod method) {
    reg::RegistrationParams p;  // tests/test_gpu_voxel_registration.py: end_to_end_params
    p.reg_type = reg::RegType::GICP;
    p.optimization_method = method;
    p.max_correspondence_distance = 1.0f;
    p.max_iterations = 30;
    p.criteria.translation = 1e-5f;
    p.criteria.rotation = 1e-5f;
    return p;
}
template <class E, class F>
static bool throws(F&& f) {
    try { f(); } catch (const E& e) { std::printf("  thrown: %s\n", e.what()); return true; } catch (...) { return false; }
    return false;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <scene file>\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t n[2] = {0, 0};
    f.read(reinterpret_cast<char*>(n), sizeof n);
    if (!f || n[0] <= 0 || n[1] <= 0) { std::printf("cannot read %s\n", argv[1]); return 2; }
    sycl_utils::DeviceQueue queue(0);
    const PointCloudCPU tgt_cpu = read_cloud(f, n[0]);
    const PointCloudCPU src_cpu = read_cloud(f, n[1]);
    if (!f) { std::printf("%s is too short\n", argv[1]); return 2; }
    const PointCloudShared target(queue, tgt_cpu), source(queue, src_cpu);
    std::printf("  target %zu points (one per voxel), source %zu points\n", target.size(), source.size());
    CHECK(target.has_cov() && source.has_cov());

    alg::mapping::VoxelHashMap map(queue, 0.5f);
    map.add_point_cloud(target, Eigen::Isometry3f::Identity());
    {
        reg::Registration gn(queue, params(reg::OptimizationMethod::GAUSS_NEWTON));
        CHECK(gn.voxel_neighbors() == 1 && !map.registration_ready(SP_REG_GICP));
        const auto r = gn.align(source, map);
        CHECK(map.registration_ready(SP_REG_GICP) && r.inlier > 0);
        std::printf("  GN, 1 cell: %zu iterations, converged %d, inlier %u, error %.6g\n", r.iterations, int(r.converged), r.inlier, r.error);
        print_pose("gn1", r.T.matrix());
        reg::Registration lm(queue, params(reg::OptimizationMethod::LEVENBERG_MARQUARDT));
        lm.set_voxel_neighbors(7);
        const auto r7 = lm.align(source, map);
        std::printf("  LM, 7 cells: %zu iterations, converged %d, inlier %u, error %.6g\n", r7.iterations, int(r7.converged), r7.inlier, r7.error);
        print_pose("lm7", r7.T.matrix());
        CHECK(r7.inlier >= r.inlier);
    }
    {
        // one Registration, two frames: the second add_point_cloud moves the map's generation, the rows are stale, align() refreshes
        alg::mapping::VoxelHashMap map2(queue, 0.5f);
        map2.add_point_cloud(target, Eigen::Isometry3f::Identity());
        reg::Registration gn(queue, params(reg::OptimizationMethod::GAUSS_NEWTON));
        const auto first = gn.align(source, map2);
        map2.add_point_cloud(target, Eigen::Isometry3f::Identity());
        CHECK(!map2.registration_ready(SP_REG_GICP));
        const auto second = gn.align(source, map2);
        CHECK(map2.registration_ready(SP_REG_GICP) && second.inlier == first.inlier);
        print_pose("gn1_second_frame", second.T.matrix());
    }
    {
        reg::Registration gn(queue, params(reg::OptimizationMethod::GAUSS_NEWTON));
        M4 guess = M4::Identity();
        guess(0, 3) = 0.25f;
        const PointCloudShared empty(queue);
        const auto r = gn.align(empty, map, guess);
        CHECK(std::memcmp(r.T.matrix().data(), guess.data(), 16 * sizeof(float)) == 0 && r.iterations == 0 && !r.converged);
        CHECK(throws<std::invalid_argument>([&] { gn.set_voxel_neighbors(5); }));
        reg::RegistrationParams p = params(reg::OptimizationMethod::GAUSS_NEWTON);
        p.reg_type = reg::RegType::POINT_TO_PLANE;
        reg::Registration plane(queue, p);
        CHECK(throws<std::invalid_argument>([&] { (void)plane.align(source, map); }));
        p = params(reg::OptimizationMethod::GAUSS_NEWTON);
        p.rotation_constraint.enable = true;
        reg::Registration rot(queue, p);
        CHECK(throws<std::invalid_argument>([&] { (void)rot.align(source, map); }));
        PointCloudCPU bare_cpu;
        *bare_cpu.points = *src_cpu.points;
        const PointCloudShared bare(queue, bare_cpu);
        CHECK(throws<std::runtime_error>([&] { (void)gn.align(bare, map); }));
    }
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
