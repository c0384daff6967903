// C++ test of registration::global_guesses with both methods through the reference's include paths. Built and run by
// tests/test_gpu_compat.py on a GPU box: test_compat_guesses <scene file>; exit code 0 = all checks passed.
// The scene file (written by that test): int32 n_source, n_target | then for the source and for the target: points (4 floats
// each) and FPFH rows (SP_FPFH_STRIDE floats each).
//   triplets            the default method: the poses as bit patterns ("T triplets<i> <16 hex words>") for the Python test
//   compatibility       method = COMPATIBILITY: every source row is a match; "T compat<i> ..."; a second call gives the same bits
//   fallback_to_mutual  the source repeated until it has more than SP_COMPAT_MAX_MATCHES rows: the method runs on the mutual
//                       matches, which are those of the first copy ("T mutual<i> ...")
//   nothing_to_match    an empty source, and descriptors of a single plane: no guesses, no throw
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
    std::vector<float> rows;
};
static Scene read_scene(std::ifstream& f, int n) {
    Scene s;
    s.cloud.points->resize(n);
    s.rows.resize(size_t(n) * SP_FPFH_STRIDE);
    f.read(reinterpret_cast<char*>(s.cloud.points->data()), sizeof(float) * 4 * n);
    f.read(reinterpret_cast<char*>(s.rows.data()), sizeof(float) * s.rows.size());
    return s;
}
static alg::feature::FPFHFeatures features_of(const sycl_utils::DeviceQueue& queue, const std::vector<float>& rows) {
    alg::feature::FPFHFeatures f;
    f.rows = std::make_shared<shared_vector<float>>(queue);
    f.rows->assign(rows.data(), rows.size());
    f.count = rows.size() / SP_FPFH_STRIDE;
    return f;
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
static reg::GlobalRegistrationParams global_params(reg::GlobalGuessMethod method) {
    reg::GlobalRegistrationParams g;  // the Python test's
    g.hypotheses = 50000;
    g.guesses = 64;
    g.inlier_distance = 1.0f;
    g.min_edge = 0.0f;
    g.edge_ratio = 0.9f;
    g.seed = 2024;
    g.method = method;
    return g;
}
static void section(const char* name, int failed_before) { std::printf("[ %s ] %s\n", g_failed == failed_before ? " OK " : "FAIL", name); }

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <scene file>\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t n[2] = {0, 0};
    f.read(reinterpret_cast<char*>(n), sizeof n);
    if (!f || n[0] <= 0 || n[1] <= 0) { std::printf("cannot read %s\n", argv[1]); return 2; }
    sycl_utils::DeviceQueue queue(0);
    const Scene src = read_scene(f, n[0]), tgt = read_scene(f, n[1]);
    if (!f) { std::printf("%s is too short\n", argv[1]); return 2; }
    const PointCloudShared source(queue, src.cloud), target(queue, tgt.cloud);
    const auto fs = features_of(queue, src.rows), ft = features_of(queue, tgt.rows);
    std::printf("  source %zu points, target %zu points\n", source.size(), target.size());
    {
        const reg::GlobalRegistrationParams defaults;
        CHECK(defaults.method == reg::GlobalGuessMethod::TRIPLETS && defaults.compat_tau == 0.1f && defaults.compat_seeds == 64 &&
              defaults.compat_k == 16 && defaults.hypotheses == 50000 && defaults.guesses == 64);
    }

    int before = g_failed;
    size_t mutual = 0;
    {
        std::vector<uint32_t> hyp;
        const auto guesses = reg::global_guesses(source, fs, target, ft, global_params(reg::GlobalGuessMethod::TRIPLETS), &hyp, &mutual);
        std::printf("  triplets: %zu matches, %zu guesses\n", mutual, guesses.size());
        CHECK(mutual >= 3 && mutual < source.size() && guesses.size() == 64 && hyp.size() == guesses.size());
        for (size_t i = 0; i < guesses.size(); ++i) print_pose("triplets" + std::to_string(i), guesses[i]);
    }
    section("triplets", before);

    before = g_failed;
    {
        std::vector<uint32_t> ranks;
        size_t matches = 0;
        const auto guesses = reg::global_guesses(source, fs, target, ft, global_params(reg::GlobalGuessMethod::COMPATIBILITY), &ranks, &matches);
        std::printf("  compatibility: %zu matches, %zu guesses\n", matches, guesses.size());
        CHECK(matches == source.size() && !guesses.empty() && guesses.size() <= 64 && ranks.size() == guesses.size());
        for (uint32_t r : ranks) CHECK(r < 64);
        for (size_t i = 0; i < guesses.size(); ++i) print_pose("compat" + std::to_string(i), guesses[i]);
        const auto again = reg::global_guesses(source, fs, target, ft, global_params(reg::GlobalGuessMethod::COMPATIBILITY));
        CHECK(again.size() == guesses.size());
        for (size_t i = 0; i < guesses.size() && i < again.size(); ++i) CHECK(same_bits(guesses[i], again[i]));
    }
    section("compatibility", before);

    before = g_failed;
    {
        Scene big;
        size_t copies = 0;
        while (big.rows.size() / SP_FPFH_STRIDE <= size_t(SP_COMPAT_MAX_MATCHES)) {
            for (size_t i = 0; i < src.cloud.size(); ++i) big.cloud.points->push_back((*src.cloud.points)[i]);
            big.rows.insert(big.rows.end(), src.rows.begin(), src.rows.end());
            ++copies;
        }
        const PointCloudShared big_source(queue, big.cloud);
        const auto big_fs = features_of(queue, big.rows);
        std::vector<uint32_t> ranks;
        size_t matches = 0;
        const auto guesses = reg::global_guesses(big_source, big_fs, target, ft, global_params(reg::GlobalGuessMethod::COMPATIBILITY), &ranks, &matches);
        std::printf("  fallback: %zu copies, %zu rows, %zu matches, %zu guesses\n", copies, big_source.size(), matches, guesses.size());
        CHECK(big_source.size() > size_t(SP_COMPAT_MAX_MATCHES) && matches == mutual && !guesses.empty());  // ties go to the first copy
        for (size_t i = 0; i < guesses.size(); ++i) print_pose("mutual" + std::to_string(i), guesses[i]);
    }
    section("fallback_to_mutual", before);

    before = g_failed;
    {
        const PointCloudShared empty(queue);
        const auto g = global_params(reg::GlobalGuessMethod::COMPATIBILITY);
        CHECK(reg::global_guesses(empty, alg::feature::FPFHFeatures(), target, ft, g).empty());
        std::vector<float> flat_s, flat_t;
        for (size_t i = 0; i < source.size(); ++i) flat_s.insert(flat_s.end(), src.rows.begin(), src.rows.begin() + SP_FPFH_STRIDE);
        for (size_t i = 0; i < target.size(); ++i) flat_t.insert(flat_t.end(), src.rows.begin(), src.rows.begin() + SP_FPFH_STRIDE);
        size_t matches = 0;
        // every source row matches target row 0: every target edge has length 0 and no two matches are compatible
        CHECK(reg::global_guesses(source, features_of(queue, flat_s), target, features_of(queue, flat_t), g, nullptr, &matches).empty());
        CHECK(matches == source.size());
        auto none = g;
        none.compat_seeds = 0;
        CHECK(reg::global_guesses(source, fs, target, ft, none).empty());
    }
    section("nothing_to_match", before);

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
