// C++ tests of knn::Octree, included through the reference's path (sycl_points/algorithms/knn/octree.hpp), after the cases of the
// reference's cpp/tests/test_octree.cpp:61-157, restated: a search against knn_search_bruteforce and the every-7th removal; then
// the accessors and exceptions, and Registration::align through the KNNBase seam against the same call with a KDTree.
// Built and run by tests/test_gpu_octree.py on a GPU box; exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

#include "sycl_points/algorithms/knn/octree.hpp"

#include "sycl_points/algorithms/common/filter_by_flags.hpp"
#include "sycl_points/algorithms/common/transform.hpp"
#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/knn/bruteforce.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"

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

static PointCloudCPU uniform_cloud(std::mt19937& gen, size_t n, float range) {
    std::uniform_real_distribution<float> coord(-range, range);
    PointCloudCPU c;
    c.points->resize(n);
    for (size_t i = 0; i < n; ++i) {
        const float x = coord(gen), y = coord(gen), z = coord(gen);
        (*c.points)[i] = PointType(x, y, z, 1.0f);
    }
    return c;
}

// rows equal bit for bit: both searches order by (distance, index)
static size_t rows_differing(const alg::knn::KNNResult& a, const alg::knn::KNNResult& b) {
    if (a.query_size != b.query_size || a.k != b.k) return size_t(-1);
    size_t bad = 0;
    for (size_t i = 0; i < a.query_size * a.k; ++i)
        bad += (*a.indices)[i] != (*b.indices)[i] || std::memcmp(&(*a.distances)[i], &(*b.distances)[i], 4) != 0;
    return bad;
}

template <class F>
static bool throws_runtime(F&& f, const char* text) {
    try { f(); } catch (const std::invalid_argument&) { return false; } catch (const std::runtime_error& e) { return std::string(e.what()) == text; }
    return false;
}

static void search_equals_bruteforce() {  // 256 targets, 64 queries, k = 4, resolution 0.1
    std::mt19937 gen(2024);
    const PointCloudCPU tc = uniform_cloud(gen, 256, 10.0f), qc = uniform_cloud(gen, 64, 10.0f);
    PointCloudShared target(*Q, tc), query(*Q, qc);
    const auto octree = alg::knn::Octree::build(*Q, target, 0.1f);
    CHECK(octree->resolution() == 0.1f && octree->max_points_per_node() == 32 && octree->size() == 256);
    CHECK(rows_differing(octree->knn_search(query, 4), alg::knn::knn_search_bruteforce(*Q, query, target, 4)) == 0);
    // k == 0 sizes the result to (nq, 0); k > 100 is refused with the reference's text
    const auto none = octree->knn_search(query, 0);
    CHECK(none.query_size == 64 && none.k == 0 && none.indices->size() == 0);
    CHECK(throws_runtime([&] { octree->knn_search(query, 101); },
                         "[Octree::knn_search_async] Requested neighbor count exceeds the supported maximum"));
    // the two-entries-per-lane list (k > 64): its first 20 columns are the brute-force rows
    const auto wide = octree->knn_search(query, 100);
    const auto bf20 = alg::knn::knn_search_bruteforce(*Q, query, target, 20);
    bool prefix = wide.k == 100 && wide.query_size == 64;
    for (size_t q = 0; prefix && q < 64; ++q)
        for (size_t j = 0; prefix && j < 20; ++j)
            prefix = (*wide.indices)[q * 100 + j] == (*bf20.indices)[q * 20 + j] && (*wide.distances)[q * 100 + j] == (*bf20.distances)[q * 20 + j];
    CHECK(prefix);
    // an octree that was never built answers with padding
    alg::knn::Octree empty(*Q, 0.1f, 32);
    const auto padded = empty.knn_search(query, 3);
    bool all_padding = padded.query_size == 64 && padded.k == 3;
    for (size_t i = 0; all_padding && i < 64 * 3; ++i)
        all_padding = (*padded.indices)[i] == -1 && (*padded.distances)[i] == std::numeric_limits<float>::max();
    CHECK(all_padding && empty.size() == 0);
}

static void removal_of_every_seventh_point() {  // 1024 points, k = 10
    std::mt19937 gen(2025);
    const size_t n = 1024, k = 10;
    const PointCloudCPU tc = uniform_cloud(gen, n, 10.0f);
    PointCloudShared target(*Q, tc);
    const auto octree = alg::knn::Octree::build(*Q, target, 0.1f);
    const auto before = octree->knn_search(target, k);
    bool self_first = true;
    for (size_t i = 0; i < n; ++i) self_first = self_first && (*before.distances)[i * k] == 0.0f && (*before.indices)[i * k] == int32_t(i);
    CHECK(self_first);

    shared_vector<uint8_t> flags(n, alg::filter::INCLUDE_FLAG, *Q);
    shared_vector<int32_t> indices(n, *Q);
    int32_t next = 0;
    for (size_t i = 0; i < n; ++i) {
        if (i % 7 == 0) flags[i] = alg::filter::REMOVE_FLAG;
        indices[i] = flags[i] == alg::filter::INCLUDE_FLAG ? next++ : -1;
    }
    shared_vector<int32_t> shorter(n - 1, *Q);
    CHECK(throws_runtime([&] { octree->remove_nodes_by_flags(flags, shorter); },
                         "[Octree::remove_nodes_by_flags] flags and indices must have the same size"));
    octree->remove_nodes_by_flags(flags, indices);
    CHECK(octree->size() == size_t(next));

    PointCloudShared kept = target;
    alg::filter::FilterByFlags filter(*Q);
    filter.filter_by_flags(*kept.points, flags);
    CHECK(kept.size() == size_t(next));
    CHECK(rows_differing(octree->knn_search(kept, k), alg::knn::knn_search_bruteforce(*Q, kept, kept, k)) == 0);
    // the id range is the compacted one now
    CHECK(throws_runtime([&] { octree->remove_nodes_by_flags(flags, indices); },
                         "[Octree::remove_nodes_by_flags] flags and indices must match the octree point identifier range"));
}

static void registration_through_the_knn_seam() {  // 2000 points, GICP: the pose a KDTree gives
    const size_t n = 2000;
    std::mt19937 gen(77);
    const PointCloudCPU tc = uniform_cloud(gen, n, 2.0f);
    PointCloudShared target(*Q, tc);
    TransformMatrix M = TransformMatrix::Identity();  // a turn of 0.03 rad about z and a small shift (column-major)
    M.data()[0] = std::cos(0.03f); M.data()[1] = std::sin(0.03f); M.data()[4] = -std::sin(0.03f); M.data()[5] = std::cos(0.03f);
    M.data()[12] = 0.03f; M.data()[13] = -0.02f; M.data()[14] = 0.01f;
    const Eigen::Isometry3f T_gt(M);
    PointCloudShared source = alg::transform::transform_copy(target, T_gt.inverse().matrix());
    std::normal_distribution<float> noise(0.0f, 0.002f);
    for (size_t i = 0; i < n; ++i) { auto& p = (*source.points)[i]; p.x() += noise(gen); p.y() += noise(gen); p.z() += noise(gen); }

    const auto tree = alg::knn::KDTree::build(*Q, target);
    const auto octree = alg::knn::Octree::build(*Q, target, 0.1f);
    alg::covariance::estimate_async(tree->knn_search(target, 10), target).wait_and_throw();
    alg::covariance::estimate_async(alg::knn::KDTree::build(*Q, source)->knn_search(source, 10), source).wait_and_throw();
    // the seed gives no tie among nearest neighbours at the initial pose: both structures list the same ones
    CHECK(rows_differing(octree->knn_search(source, 1), tree->knn_search(source, 1)) == 0);

    alg::registration::RegistrationParams p;
    p.max_iterations = 10;
    alg::registration::Registration reg(*Q, p);
    reg.set_accelerate_kdtree(false);  // both through the generic seam: KNNBase::knn_search_async per iteration
    const auto r_tree = reg.align(source, target, *tree);
    const auto r_oct = reg.align(source, target, *octree);
    float diff = 0.0f;
    for (int i = 0; i < 16; ++i) diff = std::max(diff, std::fabs(r_tree.T.matrix().data()[i] - r_oct.T.matrix().data()[i]));
    std::printf("  pose difference octree vs kdtree: %g (iterations %zu / %zu)\n", diff, r_oct.iterations, r_tree.iterations);
    CHECK(diff <= 1e-5f);
    CHECK(r_oct.inlier == r_tree.inlier && r_oct.iterations == r_tree.iterations);
    float off = 0.0f;
    for (int i = 0; i < 16; ++i) off = std::max(off, std::fabs(r_oct.T.matrix().data()[i] - T_gt.matrix().data()[i]));
    CHECK(off < 5e-3f);
}

int main() {
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(search_equals_bruteforce);
    RUN(removal_of_every_seventh_point);
    RUN(registration_through_the_knn_seam);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
