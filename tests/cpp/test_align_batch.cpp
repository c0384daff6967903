// C++ test of Registration::align_batch / best_of on the bundled pair, through the reference's include paths. Built and run by
// tests/test_gpu_align_batch.py on a GPU box: test_align_batch <golden dir>; exit code 0 = all checks passed.
// The pair is prepared as the reference's example prepares it (box filter [0.5, 50], voxel grid 0.25, k = 10 covariances), the
// target searched through a GridKNN; LM + GICP + Geman-McClure (scale 2.5), 30 iterations, convergence criteria 0 (both sides run
// to the fixed point: with a criterion two runs that differ in the last bits may stop an iteration apart).
//   1. four guesses {identity, ground truth, ground truth with a 20 degree yaw error, ground truth 5 m off} -> four results, in
//      order: four guesses are below the measured crossover of five (kAlignBatchMinGuesses), so this is align() per guess, bit
//      for bit; with two more yaw errors behind them (six guesses) it is the one launch: six results in order, identity and the
//      ground truth — inside the basin — within 1e-5 of align() from the same guess
//   2. best_of picks a result within 0.05 m / 0.01 of T_target_source.txt (the bound of tests/test_gpu_facade.py)
//   3. after the batch compute_error_frozen throws (no frozen correspondences), and works again after an align()
//   4. POINT_TO_PLANE has no batched form: the same call equals four align() calls bit for bit
// Every figure is printed before it is checked.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/filter/voxel_downsampling.hpp"
#include "sycl_points/algorithms/knn/grid.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"

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
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); std::fflush(stdout); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); std::fflush(stdout); } while (0)

static sycl_utils::DeviceQueue* Q = nullptr;
static std::string g_dir;

struct Golden {
    std::shared_ptr<PointCloudShared> source, target;
    alg::knn::GridKNN::Ptr grid;
    M4 T_gt = M4::Identity();
    std::vector<TransformMatrix> guesses;
};
static M4 rot_z(float degrees) {
    const float a = degrees * 3.14159265f / 180.0f;
    M4 m = M4::Identity();
    m(0, 0) = std::cos(a); m(0, 1) = -std::sin(a); m(1, 0) = std::sin(a); m(1, 1) = std::cos(a);
    return m;
}
static Golden& golden() {
    static Golden g;
    if (g.grid) return g;
    alg::filter::PreprocessFilter filter(*Q);
    alg::filter::VoxelGrid voxel(*Q, 0.25f);
    auto prep = [&](const std::string& name) {
        PointCloudShared scan(*Q, PointCloudReader::readFile(g_dir + "/" + name));
        filter.box_filter(scan, 0.5f, 50.0f);
        auto out = std::make_shared<PointCloudShared>(*Q);
        voxel.downsampling(scan, *out);
        const auto tree = alg::knn::KDTree::build(*Q, *out);
        alg::covariance::estimate_async(tree->knn_search(*out, 10), *out).wait_and_throw();
        alg::covariance::estimate_normals_async(tree->knn_search(*out, 10), *out).wait_and_throw();
        return out;
    };
    g.source = prep("source.ply");
    g.target = prep("target.ply");
    g.grid = alg::knn::GridKNN::build(*Q, *g.target);
    std::ifstream gt(g_dir + "/T_target_source.txt");
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) gt >> g.T_gt(r, c);
    M4 off = g.T_gt;
    off(0, 3) += 5.0f;
    g.guesses = {M4::Identity(), g.T_gt, M4(g.T_gt * rot_z(20.0f)), off};
    std::printf("  golden pair: source %zu, target %zu points\n", g.source->size(), g.target->size());
    return g;
}
static reg::RegistrationParams lm_params() {
    reg::RegistrationParams p;
    p.reg_type = reg::RegType::GICP;
    p.optimization_method = reg::OptimizationMethod::LEVENBERG_MARQUARDT;
    p.robust.type = alg::robust::RobustLossType::GEMAN_MCCLURE;
    p.robust.default_scale = 2.5f;
    p.max_iterations = 30;
    p.criteria.rotation = 0.0f;
    p.criteria.translation = 0.0f;
    return p;
}
/// max |a - b| over rows r0..r1-1, columns c0..c1-1
static float max_abs_diff(const M4& a, const M4& b, int r0 = 0, int r1 = 4, int c0 = 0, int c1 = 4) {
    float m = 0.0f;
    for (int r = r0; r < r1; ++r)
        for (int c = c0; c < c1; ++c) m = std::fmax(m, std::fabs(a(r, c) - b(r, c)));
    return m;
}

static void batch_on_the_device() {
    Golden& g = golden();
    reg::Registration batch(*Q, lm_params()), single(*Q, lm_params()), four(*Q, lm_params());
    // the one launch serves from kAlignBatchMinGuesses = 5 guesses on: the four, and two more yaw errors behind them
    CHECK(reg::Registration::kAlignBatchMinGuesses == 5);
    std::vector<TransformMatrix> six = g.guesses;
    six.push_back(M4(g.T_gt * rot_z(-10.0f)));
    six.push_back(M4(g.T_gt * rot_z(5.0f)));
    const auto results = batch.align_batch(*g.source, *g.target, *g.grid, six);
    const auto sequential = four.align_batch(*g.source, *g.target, *g.grid, g.guesses);
    CHECK(results.size() == 6 && sequential.size() == 4);
    if (results.size() != 6 || sequential.size() != 4) return;
    for (size_t i = 0; i < 4; ++i) {
        const auto ref = single.align(*g.source, *g.target, *g.grid, g.guesses[i]);
        const float d = max_abs_diff(results[i].T.matrix(), ref.T.matrix());
        std::printf("  guess %zu: batch inlier %u error %.6g iterations %zu | align inlier %u error %.6g iterations %zu | max |dT| %.3g\n", i,
                    results[i].inlier, results[i].error, results[i].iterations, ref.inlier, ref.error, ref.iterations, d);
        if (i < 2) CHECK(d <= 1e-5f);  // identity and the ground truth: inside the basin
        // four guesses are below the threshold: align() per guess
        CHECK(std::memcmp(sequential[i].T.matrix().data(), ref.T.matrix().data(), 16 * sizeof(float)) == 0 && sequential[i].inlier == ref.inlier);
    }
    const size_t best = reg::Registration::best_of(results);
    CHECK(best < 6);
    if (best >= 6) return;
    const M4 T = results[best].T.matrix();
    const float dt = max_abs_diff(T, g.T_gt, 0, 3, 3, 4), dr = max_abs_diff(T, g.T_gt, 0, 3, 0, 3);
    std::printf("  best_of -> %zu: |dt| %.4g m, |dR| %.4g against T_target_source.txt\n", best, dt, dr);
    CHECK(dt < 0.05f && dr < 0.01f);
    for (size_t i = 0; i < 6; ++i) CHECK(results[best].inlier >= results[i].inlier);
    // the batch left nothing frozen: compute_error_frozen refuses, and serves again after an align()
    bool threw = false;
    try {
        (void)batch.compute_error_frozen(*g.source, *g.target, T);
    } catch (const std::runtime_error& e) {
        threw = true;
        std::printf("  compute_error_frozen after the batch: %s\n", e.what());
    }
    CHECK(threw);
    const auto again = batch.align(*g.source, *g.target, *g.grid, g.guesses[1]);
    const auto [err, inl] = batch.compute_error_frozen(*g.source, *g.target, again.T.matrix());
    std::printf("  after align(): frozen error %.6g, inlier %u (align: %.6g, %u)\n", err, inl, again.error, again.inlier);
    CHECK(inl > 0 && std::isfinite(err));
    (void)four.compute_error_frozen(*g.source, *g.target, T);  // (the sequential path leaves align()'s correspondences)
    // fewer guesses than the threshold, and an empty list: the sequential path
    CHECK(batch.align_batch(*g.source, *g.target, *g.grid, {}).empty());
    const auto one = batch.align_batch(*g.source, *g.target, *g.grid, {g.guesses[1]});
    CHECK(one.size() == 1 && std::memcmp(one[0].T.matrix().data(), again.T.matrix().data(), 16 * sizeof(float)) == 0);
}

static void sequential_fallback() {
    Golden& g = golden();
    reg::RegistrationParams p = lm_params();
    p.reg_type = reg::RegType::POINT_TO_PLANE;
    reg::Registration batch(*Q, p), single(*Q, p);
    const auto results = batch.align_batch(*g.source, *g.target, *g.grid, g.guesses);
    CHECK(results.size() == 4);
    if (results.size() != 4) return;
    for (size_t i = 0; i < 4; ++i) {
        const auto ref = single.align(*g.source, *g.target, *g.grid, g.guesses[i]);
        const bool same = std::memcmp(results[i].T.matrix().data(), ref.T.matrix().data(), 16 * sizeof(float)) == 0 &&
                          results[i].inlier == ref.inlier && results[i].iterations == ref.iterations &&
                          std::memcmp(&results[i].error, &ref.error, sizeof(float)) == 0;
        std::printf("  POINT_TO_PLANE guess %zu: inlier %u, iterations %zu, bitwise equal to align(): %d\n", i, ref.inlier, ref.iterations, int(same));
        CHECK(same);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <golden dir>\n", argv[0]); return 2; }
    g_dir = argv[1];
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(batch_on_the_device);
    RUN(sequential_fallback);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
