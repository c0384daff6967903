// C++ tests of PreprocessFilter::weighted_random_sampling / mixed_random_sampling, included through the reference's paths only:
// the reference's thirteen weighted and mixed tests (cpp/tests/test_preprocess_filter.cpp:202-540, restated, exceptions and their
// texts included), every attribute in and out of place against the CPU restatement of the operators (sampling_restate.cpp), the
// operators' own generators across calls, and RegistrationPipeline with random_sampling.use_intensities on the golden scans.
// Built and run by tests/test_gpu_sampling.py on a GPU box (argument: the directory of the golden scans); exit code 0 = all
// checks passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/filter/voxel_downsampling.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/registration/registration_pipeline.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"

#include "sampling_restate.cpp"

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
static std::string g_golden;

static PointCloudCPU line_cloud(size_t n, float intensity0, bool with_intensity = true) {
    PointCloudCPU c;
    for (size_t i = 0; i < n; ++i) {
        c.points->push_back(PointType(float(i), 0.0f, 0.0f, 1.0f));
        if (with_intensity) c.intensities->push_back(intensity0 + float(i));
    }
    return c;
}
static shared_vector<float> weights_of(std::initializer_list<float> w) {
    shared_vector<float> v(*Q);
    v.resize(w.size());
    size_t i = 0;
    for (const float x : w) v[i++] = x;
    return v;
}
// the call throws std::invalid_argument with exactly this text
template <class Fn>
static bool throws(Fn&& fn, const char* text) {
    try { fn(); } catch (const std::invalid_argument& e) {
        if (std::strcmp(e.what(), text) != 0) std::printf("  text: %s\n", e.what());
        return std::strcmp(e.what(), text) == 0;
    }
    return false;
}
static std::vector<float> xs(const PointCloudShared& c) {
    std::vector<float> v;
    for (size_t i = 0; i < c.size(); ++i) v.push_back((*c.points)[i].x());
    return v;
}

// WeightedRandomSamplingIsDeterministicWithSeed (:202-249) — and the selection is the restatement's
static void weighted_is_deterministic_with_seed() {
    const PointCloudCPU cpu = line_cloud(5, 10.0f);
    const auto weights = weights_of({0.1f, 0.2f, 0.5f, 1.0f, 2.0f});
    PointCloudShared a(*Q, cpu), b(*Q, cpu);
    alg::filter::PreprocessFilter fa(*Q), fb(*Q);
    fa.set_random_seed(7);
    fb.set_random_seed(7);
    fa.weighted_random_sampling(a, weights, 3);
    fb.weighted_random_sampling(b, weights, 3);
    CHECK(a.size() == 3 && b.size() == 3 && a.has_intensity() && b.has_intensity());
    CHECK(xs(a) == xs(b));
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) CHECK((*a.intensities)[i] == (*b.intensities)[i]);
    const float w[5] = {0.1f, 0.2f, 0.5f, 1.0f, 2.0f};
    uint8_t flags[5];
    CHECK(sampling_weighted_restate(7, w, 5, 3, flags) == 0);
    std::vector<float> want;
    for (int i = 0; i < 5; ++i)
        if (flags[i]) want.push_back(float(i));
    CHECK(xs(a) == want);
    for (size_t i = 0; i < a.size(); ++i) CHECK((*a.intensities)[i] == (*a.points)[i].x() + 10.0f);
}

// WeightedRandomSamplingNoOpWhenSamplingCountEqualsSize (:251-278)
static void weighted_no_op_when_count_equals_size() {
    PointCloudCPU cpu = line_cloud(3, 0.5f);
    const auto weights = weights_of({1.0f, 0.0f, 2.0f});
    PointCloudShared cloud(*Q, cpu);
    alg::filter::PreprocessFilter filter(*Q);
    filter.weighted_random_sampling(cloud, weights, 3);
    CHECK(cloud.size() == 3 && cloud.has_intensity());
    CHECK((xs(cloud) == std::vector<float>{0.0f, 1.0f, 2.0f}));
    for (int i = 0; i < 3 && cloud.size() == 3; ++i) CHECK((*cloud.intensities)[i] == 0.5f + float(i));
}

// WeightedRandomSamplingCopiesOutputWhenSamplingCountCoversInput (:280-310)
static void weighted_copies_when_count_covers_input() {
    PointCloudCPU cpu = line_cloud(3, 0.5f);
    const auto weights = weights_of({1.0f, 0.0f, 2.0f});
    PointCloudShared source(*Q, cpu), output(*Q);
    output.points->resize(1);
    output.points->at(0) = PointType(99.0f, 0.0f, 0.0f, 1.0f);
    alg::filter::PreprocessFilter filter(*Q);
    filter.weighted_random_sampling(source, output, weights, 10);
    CHECK(output.size() == 3 && output.has_intensity());
    CHECK((xs(output) == std::vector<float>{0.0f, 1.0f, 2.0f}));
    for (int i = 0; i < 3 && output.size() == 3; ++i) CHECK((*output.intensities)[i] == 0.5f + float(i));
}

// WeightedRandomSamplingSkipsZeroWeightPoints (:312-334)
static void weighted_skips_zero_weight_points() {
    PointCloudShared cloud(*Q, line_cloud(4, 0.0f));
    const auto weights = weights_of({0.0f, 0.0f, 1.0f, 2.0f});
    alg::filter::PreprocessFilter filter(*Q);
    filter.set_random_seed(11);
    filter.weighted_random_sampling(cloud, weights, 2);
    CHECK((xs(cloud) == std::vector<float>{2.0f, 3.0f}));
}

// WeightedRandomSamplingThrowsWhen... (:336-418): five tests, the reference's texts
static void weighted_throws_when_count_exceeds_positive_weights() {
    PointCloudShared cloud(*Q, line_cloud(4, 0.0f, false));
    const auto weights = weights_of({0.0f, 0.0f, 1.0f, 2.0f});
    alg::filter::PreprocessFilter filter(*Q);
    CHECK(throws([&] { filter.weighted_random_sampling(cloud, weights, 3); },
                 "[PreprocessFilter::weighted_random_sampling] sampling_num exceeds positive-weight points"));
    CHECK(cloud.size() == 4);
}
static void weighted_throws_when_weight_size_mismatches() {
    PointCloudShared cloud(*Q, line_cloud(3, 0.0f, false));
    const auto weights = weights_of({1.0f, 2.0f});
    alg::filter::PreprocessFilter filter(*Q);
    CHECK(throws([&] { filter.weighted_random_sampling(cloud, weights, 2); },
                 "[PreprocessFilter::weighted_random_sampling] weights size must match points"));
}
static void weighted_throws_when_weights_contain_negative_value() {
    PointCloudShared cloud(*Q, line_cloud(3, 0.0f, false));
    const auto weights = weights_of({1.0f, -1.0f, 2.0f});
    alg::filter::PreprocessFilter filter(*Q);
    CHECK(throws([&] { filter.weighted_random_sampling(cloud, weights, 2); },
                 "[PreprocessFilter::weighted_random_sampling] weights must be finite and non-negative"));
}
static void weighted_throws_when_weights_contain_nan_or_inf() {
    PointCloudShared a(*Q, line_cloud(3, 0.0f, false)), b(*Q, line_cloud(3, 0.0f, false));
    alg::filter::PreprocessFilter filter(*Q);
    const auto nan_weights = weights_of({1.0f, std::numeric_limits<float>::quiet_NaN(), 2.0f});
    const auto inf_weights = weights_of({1.0f, std::numeric_limits<float>::infinity(), 2.0f});
    const char* text = "[PreprocessFilter::weighted_random_sampling] weights must be finite and non-negative";
    CHECK(throws([&] { filter.weighted_random_sampling(a, nan_weights, 2); }, text));
    CHECK(throws([&] { filter.weighted_random_sampling(b, inf_weights, 2); }, text));
}
static void weighted_throws_when_all_weights_are_zero() {
    PointCloudShared cloud(*Q, line_cloud(3, 0.0f, false));
    const auto weights = weights_of({0.0f, 0.0f, 0.0f});
    alg::filter::PreprocessFilter filter(*Q);
    CHECK(throws([&] { filter.weighted_random_sampling(cloud, weights, 2); },
                 "[PreprocessFilter::weighted_random_sampling] at least one weight must be positive"));
}

// MixedRandomSamplingMatchesUniformSamplingWhenWeightedRatioIsZero (:420-464)
static void mixed_matches_uniform_when_ratio_is_zero() {
    const PointCloudCPU cpu = line_cloud(5, 100.0f);
    const auto weights = weights_of({5.0f, 4.0f, 3.0f, 2.0f, 1.0f});
    PointCloudShared mixed(*Q, cpu), uniform(*Q, cpu);
    alg::filter::PreprocessFilter mf(*Q), uf(*Q);
    mf.set_random_seed(23);
    uf.set_random_seed(23);
    mf.mixed_random_sampling(mixed, weights, 3, 0.0f);
    uf.random_sampling(uniform, 3);
    CHECK(mixed.size() == 3 && uniform.size() == 3);
    CHECK(xs(mixed) == xs(uniform));
    for (size_t i = 0; i < mixed.size() && i < uniform.size(); ++i) CHECK((*mixed.intensities)[i] == (*uniform.intensities)[i]);
}

// MixedRandomSamplingFallsBackToUniformWhenWeightedPointsAreInsufficient (:466-494)
static void mixed_falls_back_to_uniform() {
    PointCloudShared cloud(*Q, line_cloud(4, 0.0f));
    const auto weights = weights_of({1.0f, 0.0f, 0.0f, 0.0f});
    alg::filter::PreprocessFilter filter(*Q);
    filter.set_random_seed(9);
    filter.mixed_random_sampling(cloud, weights, 3, 1.0f);
    CHECK(cloud.size() == 3);
    const float w[4] = {1.0f, 0.0f, 0.0f, 0.0f};
    uint8_t flags[4];
    CHECK(sampling_mixed_restate(9, w, 4, 3, 1.0f, flags) == 0);
    std::vector<float> want;
    for (int i = 0; i < 4; ++i)
        if (flags[i]) want.push_back(float(i));
    CHECK(xs(cloud) == want && want.size() == 3 && want[0] == 0.0f);
}

// MixedRandomSamplingThrowsWhenWeightedRatioIsInvalid (:496-512) — and the other two checks of the operator
static void mixed_throws_when_ratio_is_invalid() {
    PointCloudShared low(*Q, line_cloud(4, 0.0f, false)), high(*Q, line_cloud(4, 0.0f, false));
    const auto weights = weights_of({1.0f, 1.0f, 1.0f, 1.0f});
    alg::filter::PreprocessFilter filter(*Q);
    const char* text = "[PreprocessFilter::mixed_random_sampling] weighted_ratio must be within [0.0, 1.0]";
    CHECK(throws([&] { filter.mixed_random_sampling(low, weights, 2, -0.1f); }, text));
    CHECK(throws([&] { filter.mixed_random_sampling(high, weights, 2, 1.1f); }, text));
    CHECK(throws([&] { filter.mixed_random_sampling(high, weights, 2, std::numeric_limits<float>::quiet_NaN()); }, text));
    const auto few = weights_of({1.0f, 1.0f});
    CHECK(throws([&] { filter.mixed_random_sampling(low, few, 2, 0.5f); },
                 "[PreprocessFilter::mixed_random_sampling] weights size must match points"));
    const auto negative = weights_of({1.0f, 1.0f, -1.0f, 1.0f});
    CHECK(throws([&] { filter.mixed_random_sampling(low, negative, 2, 0.5f); },
                 "[PreprocessFilter::mixed_random_sampling] weights must be finite and non-negative"));
    // the reference meets the bad weight inside its loop: the two positive weights before it have drawn. The next call goes on
    // from there.
    std::mt19937 mt(1234);
    uint8_t flags[4];
    const float bad[4] = {1.0f, 1.0f, -1.0f, 1.0f}, good[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    CHECK(sampling_restate::mixed(mt, bad, 4, 2, 0.5f, flags) == 1);
    CHECK(sampling_restate::mixed(mt, good, 4, 2, 0.5f, flags) == 0);
    filter.mixed_random_sampling(low, weights, 2, 0.5f);
    std::vector<float> want;
    for (int i = 0; i < 4; ++i)
        if (flags[i]) want.push_back(float(i));
    CHECK(xs(low) == want);
}

// MixedRandomSamplingPreservesTimestampMetadataForSeparateOutput (:514-540)
static void mixed_preserves_timestamp_metadata() {
    PointCloudCPU cpu = line_cloud(5, 0.0f, false);
    cpu.start_time_ms = 2000.0;
    for (size_t i = 0; i < 5; ++i) cpu.timestamp_offsets->push_back(float(i * 10));
    cpu.end_time_ms = cpu.start_time_ms + 40.0;
    const auto weights = weights_of({1.0f, 0.5f, 0.0f, 0.0f, 2.0f});
    PointCloudShared source(*Q, cpu), output(*Q);
    alg::filter::PreprocessFilter filter(*Q);
    filter.set_random_seed(31);
    filter.mixed_random_sampling(source, output, weights, 3, 0.5f);
    CHECK(output.has_timestamps() && output.size() == 3);
    CHECK(output.start_time_ms == source.start_time_ms);
    if (output.size() == 0) return;
    const auto max_offset = *std::max_element(output.timestamp_offsets->begin(), output.timestamp_offsets->end());
    CHECK(output.end_time_ms == output.start_time_ms + static_cast<double>(max_offset));
}

// EmptyPointCloudIsNoOpForAllFilters / EmptyPointCloudClearsOutputForSamplingOperators (:542-590), the weighted parts
static void empty_cloud() {
    PointCloudCPU cpu;
    PointCloudShared cloud(*Q, cpu);
    alg::filter::PreprocessFilter filter(*Q);
    shared_vector<float> weights(*Q);
    filter.weighted_random_sampling(cloud, weights, 2);
    CHECK(cloud.size() == 0);
    filter.mixed_random_sampling(cloud, weights, 2, 0.5f);
    CHECK(cloud.size() == 0);
    PointCloudCPU stale;
    stale.points->push_back(PointType(99.0f, 0.0f, 0.0f, 1.0f));
    stale.intensities->push_back(42.0f);
    PointCloudShared output(*Q, stale);
    filter.weighted_random_sampling(cloud, output, weights, 2);
    CHECK(output.size() == 0);
}

static PointCloudCPU random_cloud(size_t n, uint32_t seed, bool timestamps) {
    std::mt19937 rs(seed);
    std::uniform_real_distribution<float> u(-20.0f, 20.0f);
    PointCloudCPU c;
    for (size_t i = 0; i < n; ++i) {
        c.points->push_back(PointType(u(rs), u(rs), u(rs), 1.0f));
        c.intensities->push_back(float(i));
        c.rgb->push_back(RGBType(u(rs), u(rs), u(rs), 1.0f));
        c.normals->push_back(Normal(u(rs), u(rs), u(rs), 0.0f));
        Covariance cv = Covariance::Zero();
        for (int k = 0; k < 9; ++k) cv((k / 3), (k % 3)) = u(rs);
        c.covs->push_back(cv);
        if (timestamps) c.timestamp_offsets->push_back(float(i % 97) * 0.5f);
    }
    return c;
}
static std::vector<float> random_weights(size_t n, uint32_t seed, float zero_share) {
    std::mt19937 rs(seed);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    std::vector<float> w(n);
    for (auto& v : w) { v = u(rs); if (u(rs) < zero_share) v = 0.0f; }
    return w;
}
static shared_vector<float> shared_weights(const std::vector<float>& w) {
    shared_vector<float> v(*Q);
    v.resize(w.size());
    for (size_t i = 0; i < w.size(); ++i) v[i] = w[i];
    return v;
}
// ulps between the m-th and the (m + 1)-th largest key of the draws a generator in state `mt` would make (a copy is advanced)
static long long threshold_gap_ulp(std::mt19937 mt, const std::vector<float>& w, size_t m) {
    std::vector<float> u;
    std::uniform_real_distribution<float> dist(std::numeric_limits<float>::min(), 1.0f);
    for (float v : w)
        if (v > 0.0f) u.push_back(dist(mt));
    std::vector<float> keys(w.size());
    sampling_keys(w.data(), u.data(), w.size(), keys.data());
    std::vector<long long> k;
    for (float v : keys) {
        if (std::isnan(v)) continue;
        int32_t b;
        std::memcpy(&b, &v, 4);
        k.push_back(b < 0 ? -(long long)(b & 0x7fffffff) : (long long)b);
    }
    if (k.size() <= m) return 1LL << 40;
    std::sort(k.begin(), k.end(), std::greater<long long>());
    return k[m - 1] - k[m];
}
// kept rows: the cloud's own order, every attribute, against the restatement's flags
static void check_rows(const PointCloudCPU& src, const PointCloudShared& out, const std::vector<uint8_t>& flags, bool ts) {
    std::vector<size_t> kept;
    for (size_t i = 0; i < flags.size(); ++i)
        if (flags[i]) kept.push_back(i);
    CHECK(out.size() == kept.size());
    if (out.size() != kept.size()) return;
    CHECK(out.has_intensity() && out.has_rgb() && out.has_normal() && out.has_cov() && out.has_timestamps() == ts);
    bool ok = true;
    float max_off = 0.0f;
    for (size_t j = 0; j < kept.size(); ++j) {
        const size_t i = kept[j];
        ok = ok && std::memcmp((*out.points)[j].data(), (*src.points)[i].data(), 16) == 0;
        ok = ok && (*out.intensities)[j] == (*src.intensities)[i];
        ok = ok && std::memcmp((*out.rgb)[j].data(), (*src.rgb)[i].data(), 16) == 0;
        ok = ok && std::memcmp((*out.normals)[j].data(), (*src.normals)[i].data(), 16) == 0;
        ok = ok && std::memcmp((*out.covs)[j].data(), (*src.covs)[i].data(), 64) == 0;
        if (ts) {
            ok = ok && (*out.timestamp_offsets)[j] == (*src.timestamp_offsets)[i];
            max_off = std::max(max_off, (*src.timestamp_offsets)[i]);
        }
    }
    CHECK(ok);
    if (ts) CHECK(out.start_time_ms == src.start_time_ms && out.end_time_ms == src.start_time_ms + double(max_off));
    else CHECK(out.start_time_ms == 0.0 && out.end_time_ms == 0.0);
}

// every attribute, in place and into another cloud, two calls in a row on one filter: the operator's generator goes on where
// the first call left it (one draw per positive weight, then the uniform draws), as the restatement's does
static void rows_and_generators() {
    const size_t n = 5000, m = 700;
    for (const bool ts : {true, false}) {
        PointCloudCPU cpu = random_cloud(n, 77, ts);
        cpu.start_time_ms = 123.0;
        const std::vector<float> w = random_weights(n, 5, 0.3f);
        const auto weights = shared_weights(w);
        alg::filter::PreprocessFilter filter(*Q);
        filter.set_random_seed(42);
        std::mt19937 wmt(42), mmt(42);
        std::vector<uint8_t> flags(n);
        for (int call = 0; call < 2; ++call) {
            CHECK(threshold_gap_ulp(wmt, w, m) > 8);
            CHECK(sampling_restate::weighted(wmt, w.data(), n, m, flags.data()) == 0);
            PointCloudShared source(*Q, cpu), output(*Q);
            if (call == 0) {
                filter.weighted_random_sampling(source, output, weights, m);
                check_rows(cpu, output, flags, ts);
                CHECK(source.size() == n);
            } else {
                filter.weighted_random_sampling(source, weights, m);
                check_rows(cpu, source, flags, ts);
            }
        }
        for (int call = 0; call < 2; ++call) {
            const float ratio = call == 0 ? 0.8f : 0.25f;
            CHECK(threshold_gap_ulp(mmt, w, size_t(std::floor(double(m) * ratio))) > 8);
            CHECK(sampling_restate::mixed(mmt, w.data(), n, m, ratio, flags.data()) == 0);
            PointCloudShared source(*Q, cpu), output(*Q);
            if (call == 0) {
                filter.mixed_random_sampling(source, output, weights, m, ratio);
                check_rows(cpu, output, flags, ts);
            } else {
                filter.mixed_random_sampling(source, weights, m, ratio);
                check_rows(cpu, source, flags, ts);
            }
        }
    }
}

// the largest difference of a translation component (returned) and of a rotation entry (*rot) from the ground truth
static float pose_distance(const Eigen::Isometry3f& T, const TransformMatrix& T_gt, float* rot) {
    const TransformMatrix M = T.matrix();
    float trans = 0.0f;
    *rot = 0.0f;
    for (int r = 0; r < 3; ++r) {
        trans = std::max(trans, std::fabs(M(r, 3) - T_gt(r, 3)));
        for (int c = 0; c < 3; ++c) *rot = std::max(*rot, std::fabs(M(r, c) - T_gt(r, c)));
    }
    return trans;
}

// RegistrationPipeline on the golden scans (the example's flow) with random_sampling.use_intensities: the registration input
// is exactly the rows the restatement selects from the source's intensities, and the pose ends as close to T_target_source.txt
// as the uniform run's does (0.05 m / 0.01 per rotation entry: what tests/test_gpu_facade.py holds the pair to).
static void pipeline_uses_intensities() {
    namespace reg = alg::registration;
    const PointCloudCPU source_cpu = PointCloudReader::readFile(g_golden + "/source.ply", false, true);
    const PointCloudCPU target_cpu = PointCloudReader::readFile(g_golden + "/target.ply", false, true);
    CHECK(source_cpu.size() > 60000 && source_cpu.intensities->size() == source_cpu.size());
    TransformMatrix T_gt = TransformMatrix::Identity();
    {
        std::ifstream f(g_golden + "/T_target_source.txt");
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) f >> T_gt(r, c);
        CHECK(bool(f));
    }
    PointCloudShared source(*Q, source_cpu), target(*Q, target_cpu), source_ds(*Q), target_ds(*Q);
    alg::filter::PreprocessFilter preprocess(*Q);
    alg::filter::VoxelGrid voxel(*Q, 0.25f);
    preprocess.box_filter(source, 0.5f, 50.0f);
    voxel.downsampling(source, source_ds);
    preprocess.box_filter(target, 0.5f, 50.0f);
    voxel.downsampling(target, target_ds);
    const auto source_tree = alg::knn::KDTree::build(*Q, source_ds);
    const auto target_tree = alg::knn::KDTree::build(*Q, target_ds);
    alg::covariance::estimate_async(source_tree->knn_search(source_ds, 10), source_ds).wait_and_throw();
    alg::covariance::estimate_async(target_tree->knn_search(target_ds, 10), target_ds).wait_and_throw();
    CHECK(source_ds.has_intensity() && source_ds.size() > 1000);

    reg::RegistrationPipelineParams pp;
    CHECK(pp.random_sampling.use_intensities == false && pp.random_sampling.weighted_ratio == 0.8f);  // the reference's defaults
    pp.registration.max_iterations = 10;
    pp.registration.max_correspondence_distance = 2.0f;
    pp.registration.optimization_method = reg::OptimizationMethod::LEVENBERG_MARQUARDT;
    pp.registration.robust.type = alg::robust::RobustLossType::GEMAN_MCCLURE;
    pp.registration.robust.default_scale = 10.0f;
    pp.registration.reg_type = reg::RegType::GICP;
    pp.robust.auto_scale = true;
    pp.robust.init_scale = 10.0f;
    pp.robust.min_scale = 2.5f;
    pp.robust.rotation_init_scale = 5.0f;
    pp.robust.rotation_min_scale = 2.5f;
    pp.robust.auto_scaling_iter = 3;
    reg::RegistrationPipeline uniform(*Q, pp);
    const auto r_uniform = uniform.align(source_ds, target_ds, *target_tree, TransformMatrix::Identity());
    pp.random_sampling.use_intensities = true;
    reg::RegistrationPipeline weighted(*Q, pp);
    const auto r_weighted = weighted.align(source_ds, target_ds, *target_tree, TransformMatrix::Identity());

    const size_t n = source_ds.size(), m = pp.random_sampling.num;
    std::vector<float> w(n);
    for (size_t i = 0; i < n; ++i) w[i] = std::as_const(*source_ds.intensities)[i];
    std::vector<uint8_t> flags(n);
    CHECK(threshold_gap_ulp(std::mt19937(1234), w, size_t(std::floor(double(m) * 0.8f))) > 8);
    CHECK(sampling_mixed_restate(1234, w.data(), n, m, 0.8f, flags.data()) == 0);
    const PointCloudShared* input = weighted.get_registration_input_point_cloud();
    CHECK(input != nullptr && input->size() == m);
    bool same = input != nullptr && input->size() == m;
    for (size_t i = 0, j = 0; same && i < n; ++i) {
        if (!flags[i]) continue;
        same = std::memcmp((*input->points)[j].data(), (*source_ds.points)[i].data(), 16) == 0 &&
               (*input->intensities)[j] == w[i] && std::memcmp((*input->covs)[j].data(), (*source_ds.covs)[i].data(), 64) == 0;
        ++j;
    }
    CHECK(same);
    CHECK(uniform.get_registration_input_point_cloud()->size() == m);
    float a_u, a_w;
    const float d_u = pose_distance(r_uniform.T, T_gt, &a_u), d_w = pose_distance(r_weighted.T, T_gt, &a_w);
    std::printf("  distance to T_target_source.txt: uniform %.4f m / %.5f, by intensity %.4f m / %.5f (translation / rotation entry)\n", d_u, a_u, d_w, a_w);
    CHECK(d_u < 0.05f && a_u < 1e-2f);
    CHECK(d_w < 0.05f && a_w < 1e-2f);
    // without intensities the flag changes nothing: the uniform path, the same rows
    PointCloudShared bare(source_ds);
    bare.intensities = std::make_shared<shared_vector<float>>(*Q);
    reg::RegistrationPipeline fallback(*Q, pp);
    pp.random_sampling.use_intensities = false;
    reg::RegistrationPipeline plain(*Q, pp);
    fallback.align(bare, target_ds, *target_tree, TransformMatrix::Identity());
    plain.align(bare, target_ds, *target_tree, TransformMatrix::Identity());
    CHECK(xs(*fallback.get_registration_input_point_cloud()) == xs(*plain.get_registration_input_point_cloud()));
}

int main(int argc, char** argv) {
    g_golden = argc > 1 ? argv[1] : "tests/golden";
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(weighted_is_deterministic_with_seed);
    RUN(weighted_no_op_when_count_equals_size);
    RUN(weighted_copies_when_count_covers_input);
    RUN(weighted_skips_zero_weight_points);
    RUN(weighted_throws_when_count_exceeds_positive_weights);
    RUN(weighted_throws_when_weight_size_mismatches);
    RUN(weighted_throws_when_weights_contain_negative_value);
    RUN(weighted_throws_when_weights_contain_nan_or_inf);
    RUN(weighted_throws_when_all_weights_are_zero);
    RUN(mixed_matches_uniform_when_ratio_is_zero);
    RUN(mixed_falls_back_to_uniform);
    RUN(mixed_throws_when_ratio_is_invalid);
    RUN(mixed_preserves_timestamp_metadata);
    RUN(empty_cloud);
    RUN(rows_and_generators);
    RUN(pipeline_uses_intensities);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
