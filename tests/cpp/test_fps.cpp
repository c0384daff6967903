// C++ tests of PreprocessFilter::farthest_point_sampling, included through the reference's paths only: the reference's own
// FPS tests (cpp/tests/test_preprocess_filter.cpp, restated), every attribute in and out of place against the CPU restatement
// of the operator (fps_restate.cpp), the time stamp rule of filter_by_flags and the operator's own generator. Built and run by
// tests/test_gpu_fps.py on a GPU box; exit code 0 = all checks passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "sycl_points/algorithms/filter/preprocess_filter.hpp"

#include "fps_restate.cpp"

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

static bool same(const Eigen::Vector4f& a, const Eigen::Vector4f& b) {
    return std::memcmp(a.data(), b.data(), sizeof(float) * 4) == 0;
}

// EmptyPointCloudIsNoOpForAllFilters / EmptyPointCloudClearsOutputForSamplingOperators (:540-590)
static void empty_cloud() {
    PointCloudCPU cpu;
    PointCloudShared cloud(*Q, cpu);
    alg::filter::PreprocessFilter filter(*Q);
    filter.farthest_point_sampling(cloud, 2);
    CHECK(cloud.size() == 0);
    PointCloudCPU stale;
    stale.points->push_back(PointType(99.0f, 0.0f, 0.0f, 1.0f));
    stale.intensities->push_back(42.0f);
    PointCloudShared output(*Q, stale);
    filter.farthest_point_sampling(cloud, output, 2);
    CHECK(output.size() == 0);
}

// FarthestPointSamplingSelectsSpreadPoints (:592-637)
static void spread_points() {
    PointCloudCPU cpu;
    const float c[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};
    for (auto& p : c) cpu.points->push_back(PointType(p[0], p[1], 0.0f, 1.0f));
    PointCloudShared cloud(*Q, cpu);
    alg::filter::PreprocessFilter filter(*Q);
    filter.set_random_seed(1234);
    filter.farthest_point_sampling(cloud, 3);
    CHECK(cloud.size() == 3);
    float max_distance = 0.0f;
    for (size_t i = 0; i < cloud.size(); ++i) {
        bool is_input = false;
        for (auto& p : c) is_input = is_input || ((*cloud.points)[i].x() == p[0] && (*cloud.points)[i].y() == p[1]);
        CHECK(is_input);
        for (size_t j = i + 1; j < cloud.size(); ++j) {
            const float dx = (*cloud.points)[i].x() - (*cloud.points)[j].x(), dy = (*cloud.points)[i].y() - (*cloud.points)[j].y();
            max_distance = std::max(max_distance, std::sqrt(dx * dx + dy * dy));
        }
    }
    CHECK(max_distance == std::sqrt(2.0f));
}

// FarthestPointSamplingCopiesOutputWhenSamplingCountCoversInput (:639-666)
static void copies_when_count_covers_input() {
    PointCloudCPU cpu;
    for (int i = 0; i < 3; ++i) {
        cpu.points->push_back(PointType(float(i), 0.0f, 0.0f, 1.0f));
        cpu.intensities->push_back(0.5f + float(i));
    }
    PointCloudShared source(*Q, cpu), output(*Q);
    output.points->resize(1);
    output.points->at(0) = PointType(99.0f, 0.0f, 0.0f, 1.0f);
    alg::filter::PreprocessFilter filter(*Q);
    filter.farthest_point_sampling(source, output, 10);
    CHECK(output.size() == 3 && output.has_intensity());
    if (output.size() != 3) return;
    for (int i = 0; i < 3; ++i) {
        CHECK((*output.points)[i].x() == float(i));
        CHECK((*output.intensities)[i] == 0.5f + float(i));
    }
    filter.farthest_point_sampling(source, output, 3);  // N == sampling_num: a copy as well
    CHECK(output.size() == 3);
}

static PointCloudCPU random_cloud(size_t n, uint32_t seed, bool timestamps) {
    std::mt19937 rs(seed);
    std::uniform_real_distribution<float> u(-20.0f, 20.0f);
    PointCloudCPU c;
    for (size_t i = 0; i < n; ++i) {
        c.points->push_back(PointType(u(rs), u(rs), u(rs), 1.0f));
        c.intensities->push_back(float(i));
        c.rgb->push_back(RGBType(u(rs), u(rs), u(rs), 1.0f));
        Normal nr(u(rs), u(rs), u(rs), 0.0f);
        c.normals->push_back(nr);
        Covariance cv = Covariance::Zero();
        for (int k = 0; k < 9; ++k) cv((k / 3), (k % 3)) = u(rs);
        c.covs->push_back(cv);
        if (timestamps) c.timestamp_offsets->push_back(float(i % 97) * 0.5f);
    }
    return c;
}

// kept rows: the cloud's own order, every attribute, against the restatement's selection
static void check_rows(const PointCloudCPU& src, const PointCloudShared& out, const std::vector<uint32_t>& order, bool ts) {
    std::vector<uint32_t> kept(order);
    std::sort(kept.begin(), kept.end());
    kept.erase(std::unique(kept.begin(), kept.end()), kept.end());
    CHECK(out.size() == kept.size());
    if (out.size() != kept.size()) return;
    CHECK(out.has_intensity() && out.has_rgb() && out.has_normal() && out.has_cov() && out.has_timestamps() == ts);
    bool ok = true;
    float max_off = 0.0f;
    for (size_t j = 0; j < kept.size(); ++j) {
        const size_t i = kept[j];
        ok = ok && same((*out.points)[j], (*src.points)[i]) && (*out.intensities)[j] == (*src.intensities)[i];
        ok = ok && same((*out.rgb)[j], (*src.rgb)[i]) && same((*out.normals)[j], (*src.normals)[i]);
        ok = ok && std::memcmp((*out.covs)[j].data(), (*src.covs)[i].data(), sizeof(float) * 16) == 0;
        if (ts) {
            ok = ok && (*out.timestamp_offsets)[j] == (*src.timestamp_offsets)[i];
            max_off = std::max(max_off, (*src.timestamp_offsets)[i]);
        }
    }
    CHECK(ok);
    if (ts) CHECK(out.end_time_ms == out.start_time_ms + double(max_off));
}

static std::vector<uint32_t> restated(const PointCloudCPU& c, size_t S, uint64_t first) {
    std::vector<uint32_t> order(S);
    std::vector<float> d(c.points->size());
    fps_restate(reinterpret_cast<const float*>(c.points->data()), c.points->size(), S, first, order.data(), d.data());
    return order;
}

static void attributes_out_of_place_and_in_place() {
    for (size_t n : {3000, 40000}) {
        const size_t S = 300;
        const PointCloudCPU cpu = random_cloud(n, 11 + (uint32_t)n, true);
        const std::vector<uint32_t> order = restated(cpu, S, fps_first_index(1234, n, 1));
        alg::filter::PreprocessFilter filter(*Q);
        PointCloudShared source(*Q, cpu), output(*Q);
        source.start_time_ms = 500.0;
        source.end_time_ms = 9999.0;
        filter.farthest_point_sampling(source, output, S);
        CHECK(source.size() == n);  // out of place: the source is left as it was
        CHECK(output.start_time_ms == 500.0);
        check_rows(cpu, output, order, true);
        // in place, a fresh filter (seed 1234 again): the same rows
        alg::filter::PreprocessFilter filter2(*Q);
        PointCloudShared data(*Q, cpu);
        data.start_time_ms = 500.0;
        filter2.farthest_point_sampling(data, S);
        check_rows(cpu, data, order, true);
        // the second call on the same filter draws the generator's second number
        const std::vector<uint32_t> order2 = restated(cpu, S, fps_first_index(1234, n, 2));
        PointCloudShared again(*Q, cpu), out2(*Q);
        again.start_time_ms = 500.0;
        filter.farthest_point_sampling(again, out2, S);
        check_rows(cpu, out2, order2, true);
    }
}

static void no_timestamps_zero_times() {
    const PointCloudCPU cpu = random_cloud(500, 5, false);
    PointCloudShared source(*Q, cpu), output(*Q);
    source.start_time_ms = 10.0;
    source.end_time_ms = 20.0;
    alg::filter::PreprocessFilter filter(*Q);
    filter.farthest_point_sampling(source, output, 50);
    check_rows(cpu, output, restated(cpu, 50, fps_first_index(1234, 500, 1)), false);
    CHECK(output.start_time_ms == 0.0 && output.end_time_ms == 0.0);  // filter_by_flags without offsets
}

// sampling_num == 0 keeps the random first point; FPS draws from a generator of its own (random_sampling does not move it);
// set_random_seed reseeds it
static void own_generator() {
    const size_t n = 1000;
    const PointCloudCPU cpu = random_cloud(n, 9, false);
    alg::filter::PreprocessFilter filter(*Q);
    PointCloudShared scratch(*Q, cpu);
    filter.random_sampling(scratch, 10);
    PointCloudShared source(*Q, cpu), output(*Q);
    filter.farthest_point_sampling(source, output, 0);
    CHECK(output.size() == 1);
    if (output.size() == 1) CHECK(same((*output.points)[0], (*cpu.points)[fps_first_index(1234, n, 1)]));
    filter.set_random_seed(77);
    filter.farthest_point_sampling(source, output, 0);
    CHECK(output.size() == 1);
    if (output.size() == 1) CHECK(same((*output.points)[0], (*cpu.points)[fps_first_index(77, n, 1)]));
}

// duplicates: the same index again once every distance is 0, so fewer points than asked come out
static void duplicates_give_fewer_points() {
    PointCloudCPU cpu;
    for (int i = 0; i < 40; ++i) cpu.points->push_back(PointType(float(i % 4), 0.0f, 0.0f, 1.0f));
    PointCloudShared cloud(*Q, cpu);
    alg::filter::PreprocessFilter filter(*Q);
    std::vector<uint32_t> order = restated(cpu, 10, fps_first_index(1234, 40, 1));
    std::sort(order.begin(), order.end());
    const size_t distinct = size_t(std::unique(order.begin(), order.end()) - order.begin());
    filter.farthest_point_sampling(cloud, 10);
    CHECK(distinct < 10 && cloud.size() == distinct);
}

int main() {
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(empty_cloud);
    RUN(spread_points);
    RUN(copies_when_count_covers_input);
    RUN(attributes_out_of_place_and_in_place);
    RUN(no_timestamps_zero_times);
    RUN(own_generator);
    RUN(duplicates_give_fewer_points);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
