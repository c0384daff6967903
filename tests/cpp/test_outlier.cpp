// C++ tests of filter::OutlierRemoval and intensity_zscore::compute, included through the reference's paths only, against the CPU
// restatement (outlier_restate.cpp, compiled into this program) on a 5 001-point cloud of noisy planes with 40 planted far points
// and every attribute, and on clouds that are too small. The bounds are tests/test_gpu_outlier.py's: per-point means, radius flags,
// z-scores and compacted attributes bit for bit; the statistical filter's threshold against float64 within 8 E_ref.
// Built (with -ffp-contract=off) and run by tests/test_gpu_outlier.py on a GPU box; exit code 0 = all checks passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/intensity_zscore.hpp"
#include "sycl_points/algorithms/filter/outlier_removal_filter.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"

#include "outlier_restate.cpp"

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
constexpr size_t kN = 5001, kPlanted = 40;

template <class F>
static bool throws_runtime(F&& f, const char* text) {
    try { f(); } catch (const std::invalid_argument&) { return false; } catch (const std::runtime_error& e) { return std::string(e.what()) == text; }
    return false;
}

// n points on three noisy planes (thickness 0.01, about 0.1 apart), then `planted` points 3 apart on a line far away; intensities
// U[0, 255), time stamps U[0, 100), colours U[0, 1)
static PointCloudCPU planes_cloud(size_t n, size_t planted, unsigned seed) {
    std::mt19937 gen(seed);
    const float side = std::sqrt(float(n) / 3.0f) * 0.1f;
    std::uniform_real_distribution<float> uv(-0.5f * side, 0.5f * side), inten(0.0f, 255.0f), stamp(0.0f, 100.0f), unit(0.0f, 1.0f);
    std::normal_distribution<float> noise(0.0f, 0.01f);
    PointCloudCPU c;
    for (size_t i = 0; i < n + planted; ++i) {
        const float a = uv(gen), b = uv(gen), d = noise(gen);
        if (i >= n) c.points->push_back(PointType(50.0f + 3.0f * float(i - n), 40.0f, 30.0f, 1.0f));
        else if (i % 3 == 0) c.points->push_back(PointType(a, b, -1.5f + d, 1.0f));
        else if (i % 3 == 1) c.points->push_back(PointType(3.0f + d, a, b, 1.0f));
        else c.points->push_back(PointType(a, -2.5f + d, b, 1.0f));
        c.intensities->push_back(inten(gen));
        c.timestamp_offsets->push_back(stamp(gen));
        c.rgb->push_back(RGBType(unit(gen), unit(gen), unit(gen), 1.0f));
    }
    return c;
}

// the planted points moved into the cloud's order (every 126th row), so that they are no suffix
static PointCloudCPU shuffled(const PointCloudCPU& in, size_t n, size_t planted, std::vector<uint8_t>& is_planted) {
    PointCloudCPU out;
    is_planted.clear();
    size_t next_planted = 0, next_regular = 0;
    for (size_t i = 0; i < n + planted; ++i) {
        const bool take_planted = next_planted < planted && (i % 126 == 7 || next_regular == n);
        const size_t src = take_planted ? n + next_planted++ : next_regular++;
        out.points->push_back((*in.points)[src]);
        out.intensities->push_back((*in.intensities)[src]);
        out.timestamp_offsets->push_back((*in.timestamp_offsets)[src]);
        out.rgb->push_back((*in.rgb)[src]);
        is_planted.push_back(take_planted);
    }
    return out;
}

template <class V>
static std::vector<unsigned char> bytes_of(const V& v) {
    const auto& h = v.host();
    const unsigned char* p = reinterpret_cast<const unsigned char*>(h.data());
    return std::vector<unsigned char>(p, p + h.size() * sizeof(typename V::value_type));
}
static std::vector<unsigned char> compact(const std::vector<unsigned char>& rows, size_t width, const std::vector<uint8_t>& flags) {
    std::vector<unsigned char> out;
    for (size_t i = 0; i < flags.size(); ++i)
        if (flags[i]) out.insert(out.end(), rows.begin() + width * i, rows.begin() + width * (i + 1));
    return out;
}

struct Before {
    std::vector<unsigned char> pts, covs, nrm, rgb, inten, stamps;
    explicit Before(const PointCloudShared& c)
        : pts(bytes_of(*c.points)), covs(bytes_of(*c.covs)), nrm(bytes_of(*c.normals)), rgb(bytes_of(*c.rgb)),
          inten(bytes_of(*c.intensities)), stamps(bytes_of(*c.timestamp_offsets)) {}
    // every attribute of `c` is the rows of this one that `flags` keeps, in order
    void check_compacted(const PointCloudShared& c, const std::vector<uint8_t>& flags) const {
        const size_t M = size_t(std::count(flags.begin(), flags.end(), uint8_t(1)));
        CHECK(c.size() == M);
        CHECK(c.has_cov() && c.has_normal() && c.has_rgb() && c.has_intensity() && c.has_timestamps());
        CHECK(bytes_of(*c.points) == compact(pts, 16, flags));
        CHECK(bytes_of(*c.covs) == compact(covs, 64, flags));
        CHECK(bytes_of(*c.normals) == compact(nrm, 16, flags));
        CHECK(bytes_of(*c.rgb) == compact(rgb, 16, flags));
        CHECK(bytes_of(*c.intensities) == compact(inten, 4, flags));
        CHECK(bytes_of(*c.timestamp_offsets) == compact(stamps, 4, flags));
    }
};

static void check_indices(const alg::filter::OutlierRemoval& f, const std::vector<uint8_t>& flags) {
    const auto& idx = f.calculate_indices().host();
    CHECK(idx.size() == flags.size());
    int32_t next = 0;
    bool ok = idx.size() == flags.size();
    for (size_t i = 0; ok && i < flags.size(); ++i) ok = idx[i] == (flags[i] ? next++ : -1);
    CHECK(ok);
}

struct Scene {
    std::vector<uint8_t> is_planted;
    PointCloudShared cloud;
    alg::knn::KDTree::Ptr tree;
    Scene() : cloud(*Q, shuffled(planes_cloud(kN, kPlanted, 61), kN, kPlanted, is_planted)) {
        tree = alg::knn::KDTree::build(*Q, cloud);
        const auto knn = tree->knn_search(cloud, 10);
        alg::covariance::estimate_async(knn, cloud).wait_and_throw();
        alg::covariance::extract_normals(cloud);
    }
};

// after remove_nodes_by_flags the tree answers as a fresh tree on the compacted cloud does: only kept points, under their new indices
static void check_tree_after_removal(const alg::knn::KDTree& tree, const PointCloudShared& cloud) {
    const auto got = tree.knn_search(cloud, 5);
    const auto want = alg::knn::KDTree::build(*Q, cloud)->knn_search(cloud, 5);
    const auto& gi = got.indices->host();
    const auto& gd = got.distances->host();
    const auto& wd = want.distances->host();
    const int32_t M = int32_t(cloud.size());
    bool in_range = gi.size() == size_t(M) * 5, same = gd.size() == wd.size(), consistent = true;
    const auto& pts = cloud.points->host();
    for (size_t e = 0; in_range && e < gi.size(); ++e) {
        in_range = gi[e] >= 0 && gi[e] < M;
        if (!in_range) break;
        const PointType &a = pts[e / 5], &b = pts[size_t(gi[e])];
        const float dx = a.x() - b.x(), dy = a.y() - b.y(), dz = a.z() - b.z();
        consistent = consistent && std::fabs(dx * dx + dy * dy + dz * dz - gd[e]) <= 1e-5f * (1.0f + gd[e]);
    }
    for (size_t e = 0; same && e < gd.size(); ++e) same = std::memcmp(&gd[e], &wd[e], 4) == 0;
    CHECK(in_range);
    CHECK(consistent);
    CHECK(same);
}

// ------------------------------------------------------------------------------------------------ statistical
static void statistical_on_planes() {
    Scene s;
    const size_t N = s.cloud.size();
    const Before before(s.cloud);
    const auto knn = s.tree->knn_search(s.cloud, 10);  // what statistical() searches itself
    const std::vector<float> d2(knn.distances->host().begin(), knn.distances->host().end());
    std::vector<float> m32(N), st32(4);
    std::vector<double> m64(N), st64(4);
    std::vector<uint8_t> f32(N), f64(N);
    outlier_statistical_restate(d2.data(), N, 10, 10, 1.0f, m32.data(), st32.data(), f32.data());
    outlier_statistical_f64(d2.data(), N, 10, 10, 1.0f, m64.data(), st64.data(), f64.data());

    alg::filter::OutlierRemoval filter(*Q);
    filter.statistical(s.cloud, *s.tree, 10, 1.0f, true);
    const std::vector<uint8_t> flags(filter.get_flags().host().begin(), filter.get_flags().host().end());
    const auto& m = filter.get_local_mean_distance().host();
    const auto& st = filter.get_statistics().host();
    CHECK(flags.size() == N && m.size() == N && st.size() == 4);
    CHECK(std::memcmp(m.data(), m32.data(), 4 * N) == 0);  // the same sequential sum
    const double e_ref = std::fabs(double(st32[2]) - st64[2]) / st64[2], e_dev = std::fabs(double(st[2]) - st64[2]) / st64[2];
    // (a handful of roundings can cancel: E_ref is taken to be at least half an ulp of the threshold)
    const double floor_ref = std::max(e_ref, 0.5 * 5.9604645e-8);
    std::printf("  threshold %.9g  E_dev = %.3e  E_ref = %.3e\n", double(st[2]), e_dev, e_ref);
    CHECK(e_dev <= 8.0 * floor_ref);
    CHECK(st[3] == float(N));
    size_t in_band = 0, wrong = 0, self = 0;
    for (size_t i = 0; i < N; ++i) {
        if (std::fabs(m64[i] - st64[2]) <= 8.0 * floor_ref * st64[2]) { ++in_band; continue; }
        wrong += flags[i] != f64[i];
        self += flags[i] != (m[i] > st[2] ? 0 : 1);
    }
    CHECK(in_band == 0);
    CHECK(wrong == 0 && self == 0);
    CHECK(flags != std::vector<uint8_t>(N, 1));
    bool exactly_planted = true;  // the 40 far points, and nothing else
    for (size_t i = 0; i < N; ++i) exactly_planted = exactly_planted && (flags[i] == 0) == (s.is_planted[i] != 0);
    CHECK(exactly_planted);
    before.check_compacted(s.cloud, flags);
    check_indices(filter, flags);
    check_tree_after_removal(*s.tree, s.cloud);
}

// ------------------------------------------------------------------------------------------------ radius
static void radius_on_planes() {
    Scene s;
    const size_t N = s.cloud.size();
    const Before before(s.cloud);
    const size_t min_k = 5;
    const float radius = 0.012f;  // against SQUARED distances of about 0.1^2: inside the distribution
    const auto knn = s.tree->knn_search(s.cloud, min_k + 1);
    const std::vector<float> d2(knn.distances->host().begin(), knn.distances->host().end());
    std::vector<uint8_t> want(N);
    outlier_radius_restate(d2.data(), N, min_k + 1, min_k, radius, want.data());
    alg::filter::OutlierRemoval filter(*Q);
    filter.radius(s.cloud, *s.tree, min_k, radius, true);
    const std::vector<uint8_t> flags(filter.get_flags().host().begin(), filter.get_flags().host().end());
    CHECK(flags == want);
    const size_t kept = size_t(std::count(flags.begin(), flags.end(), uint8_t(1)));
    std::printf("  radius kept %zu of %zu\n", kept, N);
    CHECK(kept > 0 && kept <= N - kPlanted);  // both outcomes occur
    for (size_t i = 0; i < N; ++i)
        if (s.is_planted[i]) CHECK(flags[i] == 0);
    before.check_compacted(s.cloud, flags);
    check_indices(filter, flags);
    check_tree_after_removal(*s.tree, s.cloud);
}

// ------------------------------------------------------------------------------------------------ too few points, no removal
static void too_few_points_leave_the_cloud() {
    PointCloudShared cloud(*Q, planes_cloud(7, 0, 5));
    auto tree = alg::knn::KDTree::build(*Q, cloud);
    const auto pts = bytes_of(*cloud.points);
    const auto inten = bytes_of(*cloud.intensities);
    alg::filter::OutlierRemoval filter(*Q);
    filter.statistical(cloud, *tree, 8, 1.0f);
    filter.radius(cloud, *tree, 8, 1.0f, true);
    CHECK(cloud.size() == 7 && bytes_of(*cloud.points) == pts && bytes_of(*cloud.intensities) == inten);
    CHECK(filter.get_flags().size() == 0 && filter.calculate_indices().size() == 0);
    // exactly mean_k points is enough; a huge multiplier removes nothing and every attribute survives
    filter.statistical(cloud, *tree, 7, 100.0f);
    CHECK(cloud.size() == 7 && bytes_of(*cloud.points) == pts && bytes_of(*cloud.intensities) == inten && cloud.has_timestamps());
    CHECK(filter.get_flags().size() == 7);
    PointCloudShared empty(*Q);
    filter.statistical(empty, *tree, 0, 1.0f);
    filter.radius(empty, *tree, 0, 1.0f);
    CHECK(empty.size() == 0);
}

// ------------------------------------------------------------------------------------------------ z-score
static void zscore_against_restatement() {
    for (size_t n : {size_t(5001), size_t(7), size_t(1)}) {
        PointCloudShared cloud(*Q, planes_cloud(n, 0, 71));
        auto tree = alg::knn::KDTree::build(*Q, cloud);
        const auto knn = tree->knn_search(cloud, 10);  // (7 points and 1: rows with -1 padding)
        const std::vector<int32_t> idx(knn.indices->host().begin(), knn.indices->host().end());
        const std::vector<float> inten(cloud.intensities->host().begin(), cloud.intensities->host().end());
        std::vector<float> want(n);
        intensity_zscore_restate(inten.data(), idx.data(), n, 10, 10, 0.01f, want.data());
        const auto old = cloud.intensities;
        alg::intensity_zscore::compute(cloud, knn);
        CHECK(cloud.intensities != old && cloud.intensities->size() == n);
        CHECK(std::memcmp(cloud.intensities->host().data(), want.data(), 4 * n) == 0);
        CHECK(std::memcmp(old->host().data(), inten.data(), 4 * n) == 0);  // the old vector is left as it was
    }
    // the reference's exceptions (intensity_zscore.hpp:43-53), in its order; an empty cloud returns before them
    PointCloudCPU bare;
    bare.points->push_back(PointType(1, 0, 0, 1));
    PointCloudShared no_intensity(*Q, bare);
    alg::knn::KNNResult two;
    two.allocate(*Q, 1, 2);
    CHECK(throws_runtime([&] { alg::intensity_zscore::compute(no_intensity, two); }, "[intensity_zscore::compute] Intensity field not found"));
    bare.intensities->push_back(3.0f);
    PointCloudShared one(*Q, bare);
    CHECK(throws_runtime([&] { alg::intensity_zscore::compute(one, two); }, "[intensity_zscore::compute] neighbors.k must be >= 3"));
    PointCloudShared empty(*Q);
    alg::intensity_zscore::compute(empty, two);
    CHECK(empty.size() == 0);
}

int main() {
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(statistical_on_planes);
    RUN(radius_on_planes);
    RUN(too_few_points_leave_the_cloud);
    RUN(zscore_against_restatement);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
