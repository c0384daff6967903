// C++ test of Registration::align_batch(source, VoxelHashMap&, guesses) through the reference's include paths. Built and run by
// tests/test_gpu_voxel_align_batch.py on a GPU box: test_voxel_align_batch <scene file>; exit code 0 = all checks passed.
// The scene file (written by that test): int32 n_target, n_source, n_guesses | target points (4 floats each) | target covariances
// (16 floats, column-major) | source points | source covariances | n_guesses poses and the known motion (16 floats each,
// column-major). The target is one point per 0.5 m voxel, so the map this program builds holds the very sums the map of the
// Python test holds, whatever the order of the accumulation.
//   batch_on_the_device   LM, 7 cells, the file's guesses (repeated up to kVoxelAlignBatchMinGuesses): one launch; the poses are
//                         printed as bit patterns ("T batch<i> <16 hex words>"; "R batch<i> iterations converged inlier
//                         <error bits>" for the result's scalars) and compared bit for bit with
//                         Registration.align_voxel_map_batch by the Python test; a repeated guess gives the same bits
//   sequential_fallback   with NL-Reg on the call goes guess by guess through align(source, map): the same bits as that loop
//   yaw_sweep             twelve guesses 30 degrees apart around the known motion, the first 5 degrees off: best_of ends at the
//                         known motion, with the inliers of that nearest guess
#include <cmath>
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
static void print_pose(const std::string& name, const M4& T) {
    std::printf("T %s", name.c_str());
    for (int i = 0; i < 16; ++i) {
        uint32_t w;
        std::memcpy(&w, T.data() + i, sizeof w);
        std::printf(" %08x", w);
    }
    std::printf("\n");
}
static bool same_bits(const M4& a, const M4& b) { return std::memcmp(a.data(), b.data(), 16 * sizeof(float)) == 0; }
static reg::RegistrationParams params() {
    reg::RegistrationParams p;  // tests/test_gpu_voxel_align_batch.py: test_cpp_facade
    p.reg_type = reg::RegType::GICP;
    p.optimization_method = reg::OptimizationMethod::LEVENBERG_MARQUARDT;
    p.max_correspondence_distance = 1.0f;
    p.max_iterations = 25;
    return p;
}
static void section(const char* name, int failed_before) { std::printf("[ %s ] %s\n", g_failed == failed_before ? " OK " : "FAIL", name); }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <scene file>\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t n[3] = {0, 0, 0};
    f.read(reinterpret_cast<char*>(n), sizeof n);
    if (!f || n[0] <= 0 || n[1] <= 0 || n[2] <= 0) { std::printf("cannot read %s\n", argv[1]); return 2; }
    sycl_utils::DeviceQueue queue(0);
    const PointCloudCPU tgt_cpu = read_cloud(f, n[0]);
    const PointCloudCPU src_cpu = read_cloud(f, n[1]);
    std::vector<M4> guesses(n[2]);
    for (auto& g : guesses) f.read(reinterpret_cast<char*>(g.data()), 16 * sizeof(float));
    M4 T_true;
    f.read(reinterpret_cast<char*>(T_true.data()), 16 * sizeof(float));
    if (!f) { std::printf("%s is too short\n", argv[1]); return 2; }
    const PointCloudShared target(queue, tgt_cpu), source(queue, src_cpu);
    std::printf("  target %zu points (one per voxel), source %zu points, %zu guesses\n", target.size(), source.size(), guesses.size());
    alg::mapping::VoxelHashMap map(queue, 0.5f);
    map.add_point_cloud(target, Eigen::Isometry3f::Identity());

    int before = g_failed;
    {
        std::vector<M4> many = guesses;  // (at least the facade's threshold, so that the launch is taken)
        while (many.size() < reg::Registration::kVoxelAlignBatchMinGuesses) many.push_back(guesses[many.size() % guesses.size()]);
        many.push_back(guesses[0]);
        reg::Registration lm(queue, params());
        lm.set_voxel_neighbors(7);
        CHECK(!map.registration_ready(SP_REG_GICP));
        const auto rs = lm.align_batch(source, map, many);
        CHECK(rs.size() == many.size() && map.registration_ready(SP_REG_GICP));
        for (size_t i = 0; i < guesses.size() && i < rs.size(); ++i) {
            std::printf("  guess %zu: %zu iterations, converged %d, inlier %u, error %.6g\n", i, rs[i].iterations, int(rs[i].converged),
                        rs[i].inlier, rs[i].error);
            print_pose("batch" + std::to_string(i), rs[i].T.matrix());
            uint32_t error_bits;
            std::memcpy(&error_bits, &rs[i].error, sizeof error_bits);
            std::printf("R batch%zu %zu %d %u %08x\n", i, rs[i].iterations, int(rs[i].converged), rs[i].inlier, error_bits);
            CHECK(rs[i].inlier > 0);
        }
        CHECK(same_bits(rs.back().T.matrix(), rs[0].T.matrix()) && rs.back().inlier == rs[0].inlier && rs.back().error == rs[0].error);
        CHECK(reg::Registration::best_of(rs) < rs.size());
        const PointCloudShared empty(queue);
        const auto none = lm.align_batch(empty, map, guesses);  // (an empty source: the initial guesses, as align() returns them)
        CHECK(none.size() == guesses.size() && same_bits(none[1].T.matrix(), guesses[1]));
        CHECK(lm.align_batch(source, map, {}).empty());
    }
    section("batch_on_the_device", before);

    before = g_failed;
    {
        reg::RegistrationParams p = params();
        p.degenerate_reg.type = reg::DegenerateRegularizationType::nl_reg;
        reg::Registration a(queue, p), b(queue, p);
        a.set_voxel_neighbors(7);
        b.set_voxel_neighbors(7);
        const auto rs = a.align_batch(source, map, guesses);
        CHECK(rs.size() == guesses.size());
        for (size_t i = 0; i < rs.size(); ++i) {
            const auto r = b.align(source, map, guesses[i]);
            CHECK(same_bits(rs[i].T.matrix(), r.T.matrix()) && rs[i].inlier == r.inlier && rs[i].iterations == r.iterations);
        }
    }
    section("sequential_fallback", before);

    before = g_failed;
    {
        std::vector<M4> sweep;
        for (int k = 0; k < 12; ++k) {
            const float a = (5.0f + 30.0f * k) * 3.14159265f / 180.0f;
            M4 Rz = M4::Identity();
            Rz(0, 0) = std::cos(a); Rz(0, 1) = -std::sin(a); Rz(1, 0) = std::sin(a); Rz(1, 1) = std::cos(a);
            sweep.push_back(T_true * Rz);
        }
        reg::Registration lm(queue, params());
        lm.set_voxel_neighbors(7);
        const auto rs = lm.align_batch(source, map, sweep);
        const size_t best = reg::Registration::best_of(rs);
        // (the basin is wide: the guesses next to the nearest one may end in the same optimum with the same inliers, and then the
        // last bits of the error decide among them; the guess nearest the known motion is never behind on inliers)
        CHECK(rs.size() == 12 && best < rs.size());
        if (best < rs.size()) {
            CHECK(rs[0].inlier == rs[best].inlier && rs[6].inlier < rs[best].inlier);
            const M4 Tb = rs[best].T.matrix();
            float dt = 0.0f;
            for (int r = 0; r < 3; ++r) dt += (Tb(r, 3) - T_true(r, 3)) * (Tb(r, 3) - T_true(r, 3));
            dt = std::sqrt(dt);
            std::printf("  yaw sweep: best %zu, inlier %u, %.3g m from the known motion\n", best, rs[best].inlier, dt);
            CHECK(dt < 0.05f);
        }
        for (size_t k = 0; k < rs.size(); ++k) std::printf("    %3zu deg: inlier %u, error %.5g\n", 5 + 30 * k, rs[k].inlier, rs[k].error);
    }
    section("yaw_sweep", before);

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
