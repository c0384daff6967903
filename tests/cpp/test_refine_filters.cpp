// C++ tests of the scan filters that follow kNN and covariances, included through the reference's paths only:
// PreprocessFilter::angle_incidence_filter (in place and out of place), intensity_correction::correct_intensity,
// intensity_gaussian::smooth_intensity and intensity_local_mean_norm::normalize against the CPU restatement
// (refine_restate.cpp, compiled into this program) on a 20 001-point cloud of noisy planes and on clouds of 1 and 7 points, the
// reference's exception cases (restated from cpp/tests/test_preprocess_filter.cpp:553-564, :668-720, test_intensity_correction.cpp,
// test_intensity_gaussian.cpp, test_intensity_local_mean_norm.cpp), and the refine_filter order of
// pipeline/pointcloud_processing.hpp:158-203 end to end on the bundled scan (argv[1]). The bounds are
// tests/test_gpu_refine_filters.py's: flags and compacted attributes byte for byte; intensities E_dev <= m E_ref against the
// float64 evaluation, m = 32 where pow is involved (the chain too), 6 where exp is the least accurate function.
// Built (with -ffp-contract=off) and run by tests/test_gpu_refine_filters.py on a GPU box; exit code 0 = all checks passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/intensity_correction.hpp"
#include "sycl_points/algorithms/filter/intensity_gaussian.hpp"
#include "sycl_points/algorithms/filter/intensity_local_mean_norm.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/filter/voxel_downsampling.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"

#include "refine_restate.cpp"

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
static std::string g_scan;
constexpr float kM_pow = 32.0f, kM_exp = 6.0f;
constexpr float kSaz = 0.1f, kSel = 0.1f, kSr = 0.05f;

template <class F>
static bool throws_runtime(F&& f, const char* text) {
    try { f(); } catch (const std::invalid_argument&) { return false; } catch (const std::runtime_error& e) { return std::string(e.what()) == text; }
    return false;
}
template <class F>
static bool throws_invalid(F&& f, const char* text) {
    try { f(); } catch (const std::invalid_argument& e) { return std::string(e.what()) == text; } catch (...) { return false; }
    return false;
}

// host copies of a cloud's attributes, as flat floats
struct Host {
    std::vector<float> pts, nrm, covs, inten, stamps;
    size_t n = 0;
};
static Host host_of(const PointCloudShared& c) {
    Host h;
    h.n = c.size();
    h.pts.resize(4 * h.n);
    if (h.n) std::memcpy(h.pts.data(), c.points->host().data(), 16 * h.n);
    if (c.has_normal()) { h.nrm.resize(4 * h.n); std::memcpy(h.nrm.data(), c.normals->host().data(), 16 * h.n); }
    if (c.has_cov()) { h.covs.resize(16 * h.n); std::memcpy(h.covs.data(), c.covs->host().data(), 64 * h.n); }
    if (c.has_intensity()) { h.inten.resize(h.n); std::memcpy(h.inten.data(), c.intensities->host().data(), 4 * h.n); }
    if (c.has_timestamps()) { h.stamps.resize(h.n); std::memcpy(h.stamps.data(), c.timestamp_offsets->host().data(), 4 * h.n); }
    return h;
}
static std::vector<float> compact(const std::vector<float>& rows, size_t width, const std::vector<uint8_t>& flags) {
    std::vector<float> out;
    if (rows.empty()) return out;
    for (size_t i = 0; i < flags.size(); ++i)
        if (flags[i]) out.insert(out.end(), rows.begin() + width * i, rows.begin() + width * (i + 1));
    return out;
}
static bool same_bytes(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), 4 * a.size()) == 0);
}
static std::vector<int32_t> knn_host(const alg::knn::KNNResult& r) {
    const auto& h = r.indices->host();
    return std::vector<int32_t>(h.begin(), h.end());
}
static double max_err(const std::vector<float>& a, const std::vector<double>& b) {
    double e = 0;
    for (size_t i = 0; i < a.size(); ++i)
        if (std::isfinite(b[i])) e = std::max(e, std::fabs(double(a[i]) - b[i]));
    return e;
}

// A sample of a handful of rows can by chance round every one of them exactly, and then says nothing about float32: for the
// clouds of 1 and 7 points the restatement's error is taken to be at least the final rounding it can commit, half an ulp of the
// largest result.
static double e_ref_of(const std::vector<float>& r32, const std::vector<double>& r64) {
    double e = max_err(r32, r64);
    if (r64.size() < 100) {
        float big = 0.0f;
        for (double v : r64)
            if (std::isfinite(v)) big = std::max(big, float(std::fabs(v)));
        e = std::max(e, 0.5 * double(std::nextafterf(big, INFINITY) - big));
    }
    return e;
}

// n points on three noisy planes (thickness 0.01, about 0.1 apart), intensities U[0, 255), time stamps U[0, 100)
static PointCloudCPU planes_cloud(size_t n, unsigned seed) {
    std::mt19937 gen(seed);
    const float side = std::sqrt(float(n) / 3.0f) * 0.1f;
    std::uniform_real_distribution<float> uv(-0.5f * side, 0.5f * side), inten(0.0f, 255.0f), stamp(0.0f, 100.0f);
    std::normal_distribution<float> noise(0.0f, 0.01f);
    PointCloudCPU c;
    for (size_t i = 0; i < n; ++i) {
        const float a = uv(gen), b = uv(gen), d = noise(gen);
        switch (i % 3) {
            case 0: c.points->push_back(PointType(a, b, -1.5f + d, 1.0f)); break;
            case 1: c.points->push_back(PointType(3.0f + d, a, b, 1.0f)); break;
            default: c.points->push_back(PointType(a, -2.5f + d, b, 1.0f)); break;
        }
        c.intensities->push_back(inten(gen));
        c.timestamp_offsets->push_back(stamp(gen));
    }
    return c;
}

struct Scene {
    PointCloudShared cloud;
    alg::knn::KNNResult knn;
    explicit Scene(const PointCloudCPU& cpu, bool normals) : cloud(*Q, cpu) {
        auto tree = alg::knn::KDTree::build(*Q, cloud);
        knn = tree->knn_search(cloud, 10);
        alg::covariance::estimate_async(knn, cloud).wait_and_throw();
        if (normals) alg::covariance::extract_normals(cloud);
    }
};

// ------------------------------------------------------------------------------------------------ angle of incidence
// AngleIncidenceFilterKeepsPointsWithinRange (test_preprocess_filter.cpp:668-693) and the exception cases that follow it
static void angle_filter_known_answer_and_exceptions() {
    PointCloudCPU cpu;
    cpu.points->push_back(PointType(1, 0, 0, 1));  // 0 degrees: removed
    cpu.points->push_back(PointType(1, 1, 0, 1));  // 45 degrees: kept
    cpu.points->push_back(PointType(0, 0, 1, 1));  // 90 degrees: removed
    cpu.normals->push_back(Normal(1, 0, 0, 0));
    cpu.normals->push_back(Normal(0, 1, 0, 0));
    cpu.normals->push_back(Normal(0, 1, 0, 0));
    PointCloudShared cloud(*Q, cpu);
    alg::filter::PreprocessFilter filter(*Q);
    filter.angle_incidence_filter(cloud, 0.2f, 1.2f);
    CHECK(cloud.size() == 1 && cloud.has_normal());
    CHECK((*cloud.points)[0].x() == 1.0f && (*cloud.points)[0].y() == 1.0f);
    CHECK((*cloud.normals)[0].x() == 0.0f && (*cloud.normals)[0].y() == 1.0f);

    PointCloudCPU bare;
    bare.points->push_back(PointType(1, 0, 0, 1));
    PointCloudShared no_attr(*Q, bare);
    CHECK(throws_runtime([&] { filter.angle_incidence_filter(no_attr, 0.1f, 1.0f); },
                         "[PreprocessFilter::angle_incidence_filter] Normal vector or covariance matrices must be pre-computed."));
    PointCloudShared again(*Q, cpu);
    const char* range = "[PreprocessFilter::angle_incidence_filter] Invalid angle range";
    CHECK(throws_invalid([&] { filter.angle_incidence_filter(again, -0.1f, 1.0f); }, range));
    CHECK(throws_invalid([&] { filter.angle_incidence_filter(again, 0.1f, 2.0f); }, range));
    CHECK(throws_invalid([&] { filter.angle_incidence_filter(again, 1.0f, 1.0f); }, range));
    CHECK(throws_invalid([&] { filter.angle_incidence_filter(again, 1.0f, 0.5f); }, range));
    CHECK(again.size() == 3);
    // an empty source: nothing is checked, nothing is thrown, the output is left as it is (:24-25; test :553-564)
    PointCloudShared empty(*Q), out(*Q, cpu);
    bool threw = false;
    try { filter.angle_incidence_filter(empty, 1.0f, 0.1f); filter.angle_incidence_filter(empty, out, 0.1f, 1.0f); } catch (...) { threw = true; }
    CHECK(!threw && empty.size() == 0 && out.size() == 3);
}

static void check_filtered(const PointCloudShared& got, const Host& src, const std::vector<uint8_t>& flags) {
    const Host g = host_of(got);
    CHECK(g.n == size_t(std::count(flags.begin(), flags.end(), uint8_t(1))));
    CHECK(same_bytes(g.pts, compact(src.pts, 4, flags)));
    CHECK(same_bytes(g.nrm, compact(src.nrm, 4, flags)));
    CHECK(same_bytes(g.covs, compact(src.covs, 16, flags)));
    CHECK(same_bytes(g.inten, compact(src.inten, 1, flags)));
    CHECK(same_bytes(g.stamps, compact(src.stamps, 1, flags)));
}

static void angle_filter_on_planes(size_t n) {
    PointCloudCPU cpu = planes_cloud(n, 31);
    if (n > 100) {  // a point at the origin (the NaN, Inf and zero-normal rows are planted once the attributes exist)
        (*cpu.points)[5] = PointType(0, 0, 0, 1);
    }
    Scene with_normals(cpu, true);
    PointCloudShared& cloud = with_normals.cloud;
    if (n > 100) {
        (*cloud.points)[11].x() = NAN;
        (*cloud.points)[12].y() = INFINITY;
        (*cloud.normals)[13] = Normal(0, 0, 0, 0);
    }
    const Host src = host_of(cloud);
    alg::filter::PreprocessFilter filter(*Q);
    for (const auto& band : {std::pair<float, float>(0.2f, 1.2f), std::pair<float, float>(0.0f, 1.5f)}) {
        std::vector<uint8_t> flags(n);
        angle_flags_restate(src.pts.data(), src.nrm.data(), n, band.first, band.second, flags.data());
        if (n > 100) CHECK(!flags[5] && !flags[11] && !flags[12] && !flags[13]);
        PointCloudShared out(*Q);
        filter.angle_incidence_filter(cloud, out, band.first, band.second);  // out of place
        check_filtered(out, src, flags);
        CHECK(cloud.size() == n && same_bytes(host_of(cloud).pts, src.pts));
        PointCloudShared copy(cloud);
        filter.angle_incidence_filter(copy, band.first, band.second);  // in place
        check_filtered(copy, src, flags);
    }
    // covariances only: the flags of the normals sp_normals_from_cov would store
    PointCloudShared covs_only(cloud);
    covs_only.normals->clear();
    PointCloudShared lib_normals(covs_only);
    alg::covariance::extract_normals(lib_normals);
    const Host src2 = host_of(covs_only), with_n = host_of(lib_normals);
    std::vector<uint8_t> flags(n);
    angle_flags_restate(with_n.pts.data(), with_n.nrm.data(), n, 0.2f, 1.2f, flags.data());
    filter.angle_incidence_filter(covs_only, 0.2f, 1.2f);
    CHECK(!covs_only.has_normal());
    check_filtered(covs_only, src2, flags);
}
static void angle_filter_big() { angle_filter_on_planes(20001); }
static void angle_filter_small() { angle_filter_on_planes(1); angle_filter_on_planes(7); }

// ------------------------------------------------------------------------------------------------ intensity correction
static void intensity_correction_cases() {
    // AppliesDistanceCompensation / RefDistanceNormalization / AngleCorrectionWithNormals (test_intensity_correction.cpp)
    PointCloudCPU cpu;
    cpu.points->push_back(PointType(1, 0, 0, 1));
    cpu.points->push_back(PointType(0, 3, 4, 1));
    cpu.points->push_back(PointType(1, 2, 2, 1));
    *cpu.intensities = {10.0f, 2.0f, 1.0f};
    {
        PointCloudShared c(*Q, cpu);
        alg::intensity_correction::correct_intensity(c, 2.0f, 1.0f, 0.0f, 10.0f);
        CHECK(std::fabs((*c.intensities)[0] - 10.0f) <= 1e-5f && std::fabs((*c.intensities)[1] - 10.0f) <= 1e-5f &&
              std::fabs((*c.intensities)[2] - 9.0f) <= 1e-5f);
    }
    {
        PointCloudShared c(*Q, cpu);
        alg::intensity_correction::correct_intensity(c, 2.0f, 1.0f, 0.0f, 1000.0f, 5.0f);
        CHECK(std::fabs((*c.intensities)[1] - 2.0f) <= 1e-4f && std::fabs((*c.intensities)[0] - 0.4f) <= 1e-4f);
    }
    {
        PointCloudCPU a;
        a.points->push_back(PointType(0, 0, 5, 1));
        a.points->push_back(PointType(0, 0, 5, 1));
        a.normals->push_back(Normal(0, 0, 1, 0));
        a.normals->push_back(Normal(0, std::sin(float(M_PI) / 3.0f), std::cos(float(M_PI) / 3.0f), 0));
        *a.intensities = {1.0f, 1.0f};
        PointCloudShared c(*Q, a);
        alg::intensity_correction::correct_intensity(c, 2.0f, 1.0f, 0.0f, 1000.0f, 5.0f, 1.0f);
        CHECK(std::fabs((*c.intensities)[0] - 1.0f) <= 1e-4f && std::fabs((*c.intensities)[1] - 2.0f) <= 1e-4f);
    }
    // the reference's exceptions, in its order; an empty cloud returns before them
    PointCloudShared c(*Q, cpu);
    CHECK(throws_runtime([&] { alg::intensity_correction::correct_intensity(c, -1.0f, 1.0f, 0.0f, 100.0f, 0.0f); },
                         "[correct_intensity] exponent must be non-negative"));
    CHECK(throws_runtime([&] { alg::intensity_correction::correct_intensity(c, 2.0f, 1.0f, 0.0f, 100.0f, 0.0f); },
                         "[correct_intensity] ref_distance must be positive"));
    CHECK(throws_runtime([&] { alg::intensity_correction::correct_intensity(c, 2.0f, 1.0f, 0.0f, 100.0f, -1.0f); },
                         "[correct_intensity] ref_distance must be positive"));
    cpu.intensities->clear();
    PointCloudShared no_int(*Q, cpu);
    CHECK(throws_runtime([&] { alg::intensity_correction::correct_intensity(no_int); }, "[correct_intensity] Intensity field not found"));
    PointCloudShared empty(*Q);
    bool threw = false;
    try { alg::intensity_correction::correct_intensity(empty, -1.0f); } catch (...) { threw = true; }
    CHECK(!threw);
}

static void correction_on(Scene& s, bool use_normals, float angle_exponent, const char* label) {
    PointCloudShared c(s.cloud);
    if (!use_normals) c.normals->clear();
    PointCloudShared lib_normals(c);
    if (angle_exponent != 0.0f && !use_normals) alg::covariance::extract_normals(lib_normals);
    const Host h = host_of(lib_normals);
    const size_t n = h.n;
    const float* nr = (angle_exponent != 0.0f) ? h.nrm.data() : nullptr;
    std::vector<float> r32(n);
    std::vector<double> r64(n);
    intensity_correct_restate(h.pts.data(), nr, h.inten.data(), n, 1.7f, 0.9f, 40.0f, 400.0f, 1.3f, angle_exponent, r32.data());
    intensity_correct_f64(h.pts.data(), nr, h.inten.data(), n, 1.7f, 0.9f, 40.0f, 400.0f, 1.3f, angle_exponent, r64.data());
    alg::intensity_correction::correct_intensity(c, 1.7f, 0.9f, 40.0f, 400.0f, 1.3f, angle_exponent);
    const Host got = host_of(c);
    const double E_ref = e_ref_of(r32, r64), E_dev = max_err(got.inten, r64);
    std::printf("  correction [%s, n = %zu]: E_dev = %.3e  E_ref = %.3e  m = %g\n", label, n, E_dev, E_ref, kM_pow);
    CHECK(got.n == n && E_dev <= kM_pow * E_ref);
    CHECK(same_bytes(got.pts, h.pts));
}
static void intensity_correction_against_restatement() {
    for (size_t n : {size_t(20001), size_t(1), size_t(7)}) {
        Scene s(planes_cloud(n, 41), true);
        correction_on(s, true, 0.0f, "distance");
        correction_on(s, true, 1.0f, "normals");
        correction_on(s, false, 1.0f, "covs");
    }
}

// ------------------------------------------------------------------------------------------------ smoothing, local mean
static void gaussian_cases() {
    // IsotropicSmoothingReducesVariance, NarrowRangeSigmaPreservesDepthEdge, ZenithPointsNoNaN (test_intensity_gaussian.cpp),
    // FlatIntensityYieldsUnity, MeanMinClampPreventsExplosion (test_intensity_local_mean_norm.cpp), and the exceptions of both
    auto make = [](std::vector<PointType> pts, std::vector<float> in) {
        PointCloudCPU c;
        for (auto& p : pts) c.points->push_back(p);
        *c.intensities = in;
        return c;
    };
    const std::vector<PointType> arc = {{3, -0.2f, 0, 1}, {3, -0.1f, 0, 1}, {3, 0, 0, 1}, {3, 0.1f, 0, 1}, {3, 0.2f, 0, 1}};
    {
        PointCloudShared c(*Q, make(arc, {0, 0, 1, 0, 0}));
        const auto nb = alg::knn::KDTree::build(*Q, c)->knn_search(c, 5);
        const auto before = c.intensities;
        alg::intensity_gaussian::smooth_intensity(c, nb, 0.3f, 0.3f, 0.3f);
        CHECK(c.intensities != before);  // a fresh vector was swapped in
        CHECK((*c.intensities)[2] < 1.0f && (*c.intensities)[1] > 0.0f && (*c.intensities)[3] > 0.0f);
    }
    {
        PointCloudShared c(*Q, make({{2, 0, 0, 1}, {5, 0, 0, 1}}, {1, 0}));
        const auto nb = alg::knn::KDTree::build(*Q, c)->knn_search(c, 2);
        alg::intensity_gaussian::smooth_intensity(c, nb, 1.0f, 1.0f, 0.05f);
        CHECK(std::fabs((*c.intensities)[0] - 1.0f) <= 0.01f && std::fabs((*c.intensities)[1]) <= 0.01f);
    }
    {
        PointCloudShared c(*Q, make({{0, 0, 5, 1}, {0, 0, 6, 1}, {0.1f, 0, 5, 1}}, {1, 0, 0.5f}));
        const auto nb = alg::knn::KDTree::build(*Q, c)->knn_search(c, 3);
        alg::intensity_gaussian::smooth_intensity(c, nb, 0.3f, 0.3f, 0.3f);
        for (size_t i = 0; i < 3; ++i) CHECK(std::isfinite((*c.intensities)[i]) && (*c.intensities)[i] >= 0.0f && (*c.intensities)[i] <= 1.0f);
    }
    {
        PointCloudShared c(*Q, make(arc, std::vector<float>(5, 0.5f)));
        const auto nb = alg::knn::KDTree::build(*Q, c)->knn_search(c, 5);
        alg::intensity_local_mean_norm::normalize(c, nb, 0.3f, 0.3f, 0.3f);
        for (size_t i = 0; i < 5; ++i) CHECK(std::fabs((*c.intensities)[i] - 1.0f) <= 1e-4f);
    }
    {
        PointCloudShared c(*Q, make({arc[1], arc[2], arc[3]}, {0, 0, 0}));
        const auto nb = alg::knn::KDTree::build(*Q, c)->knn_search(c, 3);
        alg::intensity_local_mean_norm::normalize(c, nb, 0.3f, 0.3f, 0.3f, 1e-3f);
        for (size_t i = 0; i < 3; ++i) CHECK((*c.intensities)[i] == 0.0f);
    }
    PointCloudShared c(*Q, make({{1, 0, 0, 1}, {1.1f, 0, 0, 1}}, {1, 0}));
    const auto nb = alg::knn::KDTree::build(*Q, c)->knn_search(c, 2);
    alg::knn::KNNResult none;
    none.allocate(*Q, 2, 0);
    const char* g = "[intensity_gaussian::smooth_intensity]";
    const char* l = "[intensity_local_mean_norm::normalize]";
    auto text = [](const char* who, const char* what) { return std::string(who) + " " + what; };
    CHECK(throws_runtime([&] { alg::intensity_gaussian::smooth_intensity(c, nb, 0.0f, 0.1f, 0.1f); }, text(g, "All sigma values must be positive").c_str()));
    CHECK(throws_runtime([&] { alg::intensity_gaussian::smooth_intensity(c, nb, 0.1f, -1.0f, 0.1f); }, text(g, "All sigma values must be positive").c_str()));
    CHECK(throws_runtime([&] { alg::intensity_gaussian::smooth_intensity(c, none, 0.1f, 0.1f); }, text(g, "neighbors.k must be >= 1").c_str()));
    CHECK(throws_runtime([&] { alg::intensity_local_mean_norm::normalize(c, nb, 0.1f, 0.1f, 0.0f); }, text(l, "All sigma values must be positive").c_str()));
    CHECK(throws_runtime([&] { alg::intensity_local_mean_norm::normalize(c, none, 0.1f, 0.1f); }, text(l, "neighbors.k must be >= 1").c_str()));
    CHECK(throws_runtime([&] { alg::intensity_local_mean_norm::normalize(c, nb, 0.1f, 0.1f, 0.1f, 0.0f); }, text(l, "mean_min must be positive").c_str()));
    CHECK(throws_runtime([&] { alg::intensity_local_mean_norm::normalize(c, nb, 0.1f, 0.0f, 0.1f, 0.0f); }, text(l, "All sigma values must be positive").c_str()));
    PointCloudCPU bare;
    bare.points->push_back(PointType(1, 0, 0, 1));
    bare.points->push_back(PointType(1.1f, 0, 0, 1));
    PointCloudShared no_int(*Q, bare);
    CHECK(throws_runtime([&] { alg::intensity_gaussian::smooth_intensity(no_int, nb, 0.1f, 0.1f); }, text(g, "Intensity field not found").c_str()));
    CHECK(throws_runtime([&] { alg::intensity_local_mean_norm::normalize(no_int, nb, 0.1f, 0.1f); }, text(l, "Intensity field not found").c_str()));
    CHECK((*c.intensities)[0] == 1.0f && (*c.intensities)[1] == 0.0f);  // nothing was changed by the calls that threw
    PointCloudShared empty(*Q);
    bool threw = false;
    try { alg::intensity_gaussian::smooth_intensity(empty, none, 0.0f, 0.0f); alg::intensity_local_mean_norm::normalize(empty, none, 0.0f, 0.0f, 0.0f, 0.0f); } catch (...) { threw = true; }
    CHECK(!threw);
}

static void gaussian_against_restatement() {
    for (size_t n : {size_t(20001), size_t(1), size_t(7)}) {
        Scene s(planes_cloud(n, 53), false);
        const Host h = host_of(s.cloud);
        const std::vector<int32_t> knn = knn_host(s.knn);
        CHECK(knn.size() == 10 * n);
        if (n == 7) CHECK(knn[7] == -1 && knn[9] == -1);  // the padding of a cloud with fewer than k points
        for (const float mean_min : {0.0f, 1e-3f})
            for (const size_t k_limit : {size_t(0), size_t(4)}) {
                const size_t k_use = k_limit ? k_limit : 10;
                std::vector<float> r32(n);
                std::vector<double> r64(n);
                intensity_gaussian_restate(h.pts.data(), h.inten.data(), knn.data(), n, 10, k_use, kSaz, kSel, kSr, mean_min, r32.data(), nullptr, nullptr);
                intensity_gaussian_f64(h.pts.data(), h.inten.data(), knn.data(), n, 10, k_use, kSaz, kSel, kSr, mean_min, r64.data(), nullptr, nullptr);
                PointCloudShared c(s.cloud);
                if (mean_min > 0.0f) alg::intensity_local_mean_norm::normalize(c, s.knn, kSaz, kSel, kSr, mean_min, k_limit);
                else alg::intensity_gaussian::smooth_intensity(c, s.knn, kSaz, kSel, kSr, k_limit);
                const Host got = host_of(c);
                const double E_ref = e_ref_of(r32, r64), E_dev = max_err(got.inten, r64);
                std::printf("  %s [n = %zu, k_use = %zu]: E_dev = %.3e  E_ref = %.3e  m = %g\n", mean_min > 0.0f ? "local mean" : "smoothing ", n,
                            k_use, E_dev, E_ref, kM_exp);
                CHECK(got.n == n && got.inten.size() == n && E_dev <= kM_exp * E_ref);
            }
    }
}

// ------------------------------------------------------------------------------------------------ refine_filter, end to end
// pipeline/pointcloud_processing.hpp:158-203 after its two earlier stages: box filter, 0.25 voxels, k = 10 covariances; then the
// angle filter, the correction, the smoothing and the normalisation, each on the result of the one before. The scan has no
// intensity channel, so one is made up from the position. The filtered cloud's neighbours are searched again (the indices of the
// search before the filter name rows of the cloud before it). The restatement is chained the same way in float and — each
// stage in double on the previous stage's result rounded to float — as the yardstick.
static void end_to_end() {
    PointCloudCPU scan = PointCloudReader::readFile(g_scan);
    CHECK(scan.size() > 10000);
    scan.intensities->resize(scan.size());
    for (size_t i = 0; i < scan.size(); ++i) {
        const PointType& p = (*scan.points)[i];
        (*scan.intensities)[i] = 20.0f + 100.0f * (1.0f + std::sin(3.0f * p.x()) * std::cos(2.0f * p.y() + p.z()));
    }
    PointCloudShared raw(*Q, scan), boxed(*Q), cloud(*Q);
    alg::filter::PreprocessFilter pre(*Q);
    pre.box_filter(raw, boxed, 1.0f, 50.0f);
    alg::filter::VoxelGrid vg(*Q, 0.25f);
    vg.downsampling(boxed, cloud);
    CHECK(cloud.has_intensity() && cloud.size() > 1000);
    auto tree = alg::knn::KDTree::build(*Q, cloud);
    const auto nb = tree->knn_search(cloud, 10);
    alg::covariance::estimate_async(nb, cloud).wait_and_throw();
    // the host's copy of the stage's input, with the normals the covariance path uses
    PointCloudShared lib_normals(cloud);
    alg::covariance::extract_normals(lib_normals);
    const Host in = host_of(lib_normals);
    const size_t n0 = in.n;

    const float lo_a = 0.1f, hi_a = 1.45f, s_az = 0.5f, s_el = 0.5f, s_r = 0.2f;
    pre.angle_incidence_filter(cloud, cloud, lo_a, hi_a);
    std::vector<uint8_t> flags(n0);
    angle_flags_restate(in.pts.data(), in.nrm.data(), n0, lo_a, hi_a, flags.data());
    const std::vector<float> pts = compact(in.pts, 4, flags), nrm = compact(in.nrm, 4, flags);
    const size_t n = pts.size() / 4;
    std::printf("  end to end: %zu points in, %zu after the angle filter\n", n0, n);
    CHECK(cloud.size() == n && n > 500 && n < n0);
    CHECK(same_bytes(host_of(cloud).pts, pts));
    if (cloud.size() != n) return;

    alg::intensity_correction::correct_intensity(cloud, 2.0f, 1.0f, 0.0f, 1000.0f, 10.0f, 1.0f);
    auto tree2 = alg::knn::KDTree::build(*Q, cloud);
    const auto nb2 = tree2->knn_search(cloud, 10);
    alg::intensity_gaussian::smooth_intensity(cloud, nb2, s_az, s_el, s_r, 8);
    alg::intensity_local_mean_norm::normalize(cloud, nb2, s_az, s_el, s_r, 1e-3f, 8);
    const Host got = host_of(cloud);
    const std::vector<int32_t> knn = knn_host(nb2);

    const std::vector<float> i0 = compact(in.inten, 1, flags);
    std::vector<float> a32(n), b32(n), c32(n), a64f(n), b64f(n);
    std::vector<double> a64(n), b64(n), c64(n);
    intensity_correct_restate(pts.data(), nrm.data(), i0.data(), n, 2.0f, 1.0f, 0.0f, 1000.0f, 10.0f, 1.0f, a32.data());
    intensity_gaussian_restate(pts.data(), a32.data(), knn.data(), n, 10, 8, s_az, s_el, s_r, 0.0f, b32.data(), nullptr, nullptr);
    intensity_gaussian_restate(pts.data(), b32.data(), knn.data(), n, 10, 8, s_az, s_el, s_r, 1e-3f, c32.data(), nullptr, nullptr);
    intensity_correct_f64(pts.data(), nrm.data(), i0.data(), n, 2.0f, 1.0f, 0.0f, 1000.0f, 10.0f, 1.0f, a64.data());
    for (size_t i = 0; i < n; ++i) a64f[i] = float(a64[i]);
    intensity_gaussian_f64(pts.data(), a64f.data(), knn.data(), n, 10, 8, s_az, s_el, s_r, 0.0f, b64.data(), nullptr, nullptr);
    for (size_t i = 0; i < n; ++i) b64f[i] = float(b64[i]);
    intensity_gaussian_f64(pts.data(), b64f.data(), knn.data(), n, 10, 8, s_az, s_el, s_r, 1e-3f, c64.data(), nullptr, nullptr);
    const double E_ref = max_err(c32, c64), E_dev = max_err(got.inten, c64);
    std::printf("  end to end: E_dev = %.3e  E_ref = %.3e  m = %g\n", E_dev, E_ref, kM_pow);
    CHECK(got.inten.size() == n && E_ref > 0.0 && E_dev <= kM_pow * E_ref);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: test_refine_filters <scan.ply>\n"); return 2; }
    g_scan = argv[1];
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(angle_filter_known_answer_and_exceptions);
    RUN(angle_filter_big);
    RUN(angle_filter_small);
    RUN(intensity_correction_cases);
    RUN(intensity_correction_against_restatement);
    RUN(gaussian_cases);
    RUN(gaussian_against_restatement);
    RUN(end_to_end);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
