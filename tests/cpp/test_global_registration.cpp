// C++ test of feature::compute_fpfh / registration::global_guesses / Registration::align_global through the reference's include
// paths. Built and run by tests/test_gpu_global_registration.py on a GPU box:
// test_global_registration <scene file>; exit code 0 = all checks passed.
// The scene file (written by that test): int32 n_source, n_target, k | then for the source and for the target: points (4 floats
// each), normals (4), covariances (16, column-major), the cloud's own k-NN indices (k int32 per point) and squared distances.
//   descriptors     FPFH rows of both clouds; their bytes as a checksum ("F <name> <fnv1a-64>") for the Python test
//   guesses         global_guesses: the poses as bit patterns ("T guess<i> <16 hex words>"), compared bit for bit with
//                   Registration.align_global's guesses by the Python test; a second call gives the same bits
//   align_global    the winner ("T winner ..."; "R winner iterations converged inlier <error bits>") against a GridKNN target
//   nothing_to_match  an empty source, and descriptors of a single plane: converged == false, the identity, no throw
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

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

struct Scene {
    PointCloudCPU cloud;
    std::vector<int32_t> idx;
    std::vector<float> d2;
};
static Scene read_scene(std::ifstream& f, int n, int k) {
    Scene s;
    s.cloud.points->resize(n);
    s.cloud.normals->resize(n);
    s.cloud.covs->resize(n);
    s.idx.resize(size_t(n) * k);
    s.d2.resize(size_t(n) * k);
    f.read(reinterpret_cast<char*>(s.cloud.points->data()), sizeof(float) * 4 * n);
    f.read(reinterpret_cast<char*>(s.cloud.normals->data()), sizeof(float) * 4 * n);
    f.read(reinterpret_cast<char*>(s.cloud.covs->data()), sizeof(float) * 16 * n);
    f.read(reinterpret_cast<char*>(s.idx.data()), sizeof(int32_t) * s.idx.size());
    f.read(reinterpret_cast<char*>(s.d2.data()), sizeof(float) * s.d2.size());
    return s;
}
static alg::knn::KNNResult lists_of(const sycl_utils::DeviceQueue& queue, const Scene& s, int k) {
    alg::knn::KNNResult r;
    r.allocate(queue, 0, 0, false);
    r.indices->assign(s.idx.data(), s.idx.size());
    r.distances->assign(s.d2.data(), s.d2.size());
    r.query_size = s.cloud.size();
    r.k = size_t(k);
    return r;
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
static uint64_t checksum(const alg::feature::FPFHFeatures& f) {
    const auto& host = f.rows->host();
    uint64_t h = 1469598103934665603ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(host.data());
    for (size_t i = 0; i < host.size() * sizeof(float); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
static reg::RegistrationParams params() {
    reg::RegistrationParams p;  // tests/test_gpu_global_registration.py: registration()
    p.reg_type = reg::RegType::GICP;
    p.max_correspondence_distance = 2.0f;
    p.max_iterations = 30;
    return p;
}
static reg::GlobalRegistrationParams global_params() {
    reg::GlobalRegistrationParams g;  // the Python test's
    g.hypotheses = 50000;
    g.guesses = 64;
    g.inlier_distance = 1.0f;
    g.min_edge = 0.0f;
    g.edge_ratio = 0.9f;
    g.seed = 2024;
    return g;
}
static void section(const char* name, int failed_before) { std::printf("[ %s ] %s\n", g_failed == failed_before ? " OK " : "FAIL", name); }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <scene file>\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t n[3] = {0, 0, 0};
    f.read(reinterpret_cast<char*>(n), sizeof n);
    if (!f || n[0] <= 0 || n[1] <= 0 || n[2] <= 0 || n[2] > 64) { std::printf("cannot read %s\n", argv[1]); return 2; }
    sycl_utils::DeviceQueue queue(0);
    const Scene src = read_scene(f, n[0], n[2]), tgt = read_scene(f, n[1], n[2]);
    if (!f) { std::printf("%s is too short\n", argv[1]); return 2; }
    const PointCloudShared source(queue, src.cloud), target(queue, tgt.cloud);
    std::printf("  source %zu points, target %zu points, k = %d\n", source.size(), target.size(), n[2]);

    int before = g_failed;
    const auto fs = alg::feature::compute_fpfh(lists_of(queue, src, n[2]), source);
    const auto ft = alg::feature::compute_fpfh(lists_of(queue, tgt, n[2]), target);
    CHECK(fs.size() == source.size() && ft.size() == target.size() && fs.rows->size() == source.size() * SP_FPFH_STRIDE);
    std::printf("F source %016llx\nF target %016llx\n", (unsigned long long)checksum(fs), (unsigned long long)checksum(ft));
    section("descriptors", before);

    before = g_failed;
    std::vector<uint32_t> hyp;
    size_t matches = 0;
    const auto guesses = reg::global_guesses(source, fs, target, ft, global_params(), &hyp, &matches);
    std::printf("  %zu matches, %zu guesses\n", matches, guesses.size());
    CHECK(matches >= 3 && guesses.size() == 64 && hyp.size() == guesses.size());
    for (size_t i = 0; i < guesses.size(); ++i) print_pose("guess" + std::to_string(i), guesses[i]);
    const auto again = reg::global_guesses(source, fs, target, ft, global_params());
    CHECK(again.size() == guesses.size());
    for (size_t i = 0; i < guesses.size() && i < again.size(); ++i) CHECK(same_bits(guesses[i], again[i]));
    section("guesses", before);

    before = g_failed;
    const auto grid = alg::knn::GridKNN::build(queue, target);
    {
        reg::Registration r(queue, params());
        std::vector<reg::RegistrationResult> all;
        std::vector<M4> used;
        const auto res = r.align_global(source, fs, target, ft, *grid, global_params(), &all, &used);
        CHECK(res.converged && res.inlier > 0 && all.size() == 64 && used.size() == 64);
        for (size_t i = 0; i < used.size() && i < guesses.size(); ++i) CHECK(same_bits(used[i], guesses[i]));
        print_pose("winner", res.T.matrix());
        uint32_t error_bits;
        std::memcpy(&error_bits, &res.error, sizeof error_bits);
        std::printf("R winner %zu %d %u %08x\n", res.iterations, int(res.converged), res.inlier, error_bits);
    }
    section("align_global", before);

    before = g_failed;
    {
        reg::Registration r(queue, params());
        const PointCloudShared empty(queue);
        const auto none = r.align_global(empty, alg::feature::FPFHFeatures(), target, ft, *grid, global_params());
        CHECK(!none.converged && same_bits(none.T.matrix(), M4::Identity()));
        // a single plane: every point carries the same descriptor, one mutual pair survives
        alg::feature::FPFHFeatures flat_s = fs, flat_t = ft;
        flat_s.rows = std::make_shared<shared_vector<float>>(queue);
        flat_t.rows = std::make_shared<shared_vector<float>>(queue);
        const auto& row = fs.rows->host();
        std::vector<float> tiled;
        for (size_t i = 0; i < std::max(source.size(), target.size()); ++i) tiled.insert(tiled.end(), row.begin(), row.begin() + SP_FPFH_STRIDE);
        flat_s.rows->assign(tiled.data(), source.size() * SP_FPFH_STRIDE);
        flat_t.rows->assign(tiled.data(), target.size() * SP_FPFH_STRIDE);
        CHECK(reg::match_features(queue, flat_s, flat_t).size() == 1);
        std::vector<reg::RegistrationResult> all;
        const auto flat = r.align_global(source, flat_s, target, flat_t, *grid, global_params(), &all);
        CHECK(!flat.converged && same_bits(flat.T.matrix(), M4::Identity()) && all.empty());
    }
    section("nothing_to_match", before);

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
