// C++ test of what the facade does "to every attribute the cloud carries", on clouds that carry SOME of the optional attributes:
// all 32 subsets of {covs, normals, rgb, intensities, timestamp_offsets}, N = 1 (one row), 64 (a full wave), 65, 257 (one over the
// 256-lane block) and 1030 (more than four blocks). Row i of every present attribute carries the tag i, so rows that go out of step
// show. box_filter, random_sampling, angle_incidence_filter (out of place and in place), OutlierRemoval::radius, erase, extend, the
// copy constructor, VoxelGrid and PolarGrid. Every comparison is exact: rows are moved, not computed; the downsampling grids see
// one point per voxel, so their output is a permutation of the input.
// Built and run by tests/test_gpu_cloud_rows.py on a GPU box; exit code 0 = all checks passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#include "sycl_points/algorithms/filter/outlier_removal_filter.hpp"
#include "sycl_points/algorithms/filter/polar_downsampling.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/filter/voxel_downsampling.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"

using namespace sycl_points;
namespace alg = sycl_points::algorithms;

static int g_failed = 0, g_checks = 0;
static size_t g_n = 0;
static unsigned g_mask = 0;
#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        ++g_checks;                                                                                                              \
        if (!(cond) && ++g_failed <= 40) std::printf("  CHECK FAILED %s:%d  N=%zu mask=%u  %s\n", __FILE__, __LINE__, g_n, g_mask, #cond); \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); const int before = g_failed; every_cloud(fn); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); } while (0)

static sycl_utils::DeviceQueue* Q = nullptr;
enum : unsigned { COV = 1, NRM = 2, RGB = 4, INTEN = 8, STAMPS = 16, ALL = 31 };
constexpr double kStart = 500.0, kEnd = 9999.0;  // the tagged cloud's times
constexpr float kMinAngle = 0.2f, kMaxAngle = 1.2f;

template <class F>
static void every_cloud(F&& f) {
    for (size_t n : {1, 64, 65, 257, 1030})
        for (unsigned mask = 0; mask <= ALL; ++mask) {
            g_n = n;
            g_mask = mask;
            f(n, mask);
        }
}

// Point i: the largest coordinate (the box filter's distance) is y = 1.25 + i, so the tag can be read off the point. Odd points lie
// at 45 degrees to the x axis, even ones at 89.4: with the normal along x (the cloud's normals (i, 0, 0), or the smallest axis of
// its covariances diag(i, 2000, 3000)) the angle of incidence keeps the odd ones, far from both bounds. Point 0 has a zero normal.
static PointCloudCPU tagged_cloud(size_t n, unsigned mask) {
    PointCloudCPU c;
    for (size_t i = 0; i < n; ++i) {
        const float tag = float(i), s = 1.25f + tag;
        c.points->push_back(PointType(i % 2 ? s : 0.01f * s, s, 0.0f, 1.0f));
        if (mask & COV) {
            Covariance m = Covariance::Zero();
            m(0, 0) = tag; m(1, 1) = 2000.0f; m(2, 2) = 3000.0f;
            c.covs->push_back(m);
        }
        if (mask & NRM) c.normals->push_back(Normal(tag, 0.0f, 0.0f, 0.0f));
        if (mask & RGB) c.rgb->push_back(RGBType(tag, 0.5f, 0.25f, 1.0f));
        if (mask & INTEN) c.intensities->push_back(tag);
        if (mask & STAMPS) c.timestamp_offsets->push_back(tag);
    }
    c.start_time_ms = kStart;
    c.end_time_ms = kEnd;
    return c;
}
// what an out-of-place call writes into: three rows of every attribute and times of its own
static PointCloudShared used_output() {
    PointCloudShared out(*Q, tagged_cloud(3, ALL));
    out.start_time_ms = 1.0;
    out.end_time_ms = 2.0;
    return out;
}
static bool times_are(const PointCloudShared& c, double t0, double t1) { return c.start_time_ms == t0 && c.end_time_ms == t1; }
static float tag_of(const PointType& p) { return p.y() - 1.25f; }

// `c` holds the rows `want` (tags, in order) of the tagged cloud: the points themselves; every attribute of `mask` with as many rows
// as points, row j carrying point j's tag; the other attributes empty. exact_points: the points are the cloud's, bit for bit
static void check_rows(const PointCloudShared& c, unsigned mask, const std::vector<uint32_t>& want, bool exact_points = true) {
    const size_t M = want.size();
    const auto& p = c.points->host();
    bool ok = p.size() == M;
    for (size_t j = 0; ok && j < M; ++j) {
        const float s = 1.25f + float(want[j]);
        ok = tag_of(p[j]) == float(want[j]);
        if (exact_points) ok = ok && p[j].x() == (want[j] % 2 ? s : 0.01f * s) && p[j].y() == s && p[j].z() == 0.0f && p[j].w() == 1.0f;
    }
    CHECK(ok);
    auto attribute = [&](unsigned bit, const auto& v, auto&& tag) {
        const auto& h = v.host();
        bool rows = h.size() == ((mask & bit) ? M : 0);
        for (size_t j = 0; rows && j < h.size(); ++j) rows = tag(h[j]) == float(want[j]);
        return rows;
    };
    CHECK(attribute(COV, *c.covs, [](const Covariance& m) { return m(0, 0); }));
    CHECK(attribute(NRM, *c.normals, [](const Normal& v) { return v.x(); }));
    CHECK(attribute(RGB, *c.rgb, [](const RGBType& v) { return v.x(); }));
    CHECK(attribute(INTEN, *c.intensities, [](float v) { return v; }));
    CHECK(attribute(STAMPS, *c.timestamp_offsets, [](float v) { return v; }));
    const unsigned has = (c.has_cov() ? COV : 0) | (c.has_normal() ? NRM : 0) | (c.has_rgb() ? RGB : 0) |
                         (c.has_intensity() ? INTEN : 0) | (c.has_timestamps() ? STAMPS : 0);
    CHECK(has == (M ? mask : 0u));
}
static bool strictly_increasing(const std::vector<uint32_t>& v) {
    return std::adjacent_find(v.begin(), v.end(), std::greater_equal<uint32_t>()) == v.end();
}
template <class Keep>
static std::vector<uint32_t> kept_by(size_t n, Keep&& keep) {
    std::vector<uint32_t> want;
    for (size_t i = 0; i < n; ++i)
        if (keep(i)) want.push_back(uint32_t(i));
    return want;
}

// out of place (into a used cloud: every attribute is replaced, the times are the source's) and in place
template <class Op>
static void both_ways(size_t n, unsigned mask, const std::vector<uint32_t>& want, Op&& op) {
    CHECK(strictly_increasing(want));
    const PointCloudCPU cpu = tagged_cloud(n, mask);
    PointCloudShared source(*Q, cpu), output = used_output();
    op(source, output);
    check_rows(output, mask, want);
    CHECK(times_are(output, kStart, kEnd));
    std::vector<uint32_t> all(n);
    std::iota(all.begin(), all.end(), 0u);
    check_rows(source, mask, all);  // the source is left as it was
    PointCloudShared data(*Q, cpu);
    op(data, data);
    check_rows(data, mask, want);
    CHECK(times_are(data, kStart, kEnd));
}

// the box filter keeps min <= largest |coordinate| <= max: a middle band, everything, nothing
static void box_filter_rows(size_t n, unsigned mask) {
    const std::pair<float, float> bands[] = {{1.0f + float(n / 4), 1.0f + float(3 * n / 4)},
                                             {0.0f, std::numeric_limits<float>::max()},
                                             {1.0e6f, 2.0e6f}};
    for (const auto& [lo, hi] : bands) {
        const auto want = kept_by(n, [&, lo = lo, hi = hi](size_t i) { return 1.25f + float(i) >= lo && 1.25f + float(i) <= hi; });
        alg::filter::PreprocessFilter filter(*Q);
        both_ways(n, mask, want, [&, lo = lo, hi = hi](PointCloudShared& in, PointCloudShared& out) { filter.box_filter(in, out, lo, hi); });
    }
}

// the partial Fisher-Yates of random_sampling_operator.hpp:24-51 on the filters' seed (1234), the sample in the cloud's order; each
// of the two calls has a fresh filter, so both draw the same rows
static void random_sampling_rows(size_t n, unsigned mask) {
    const size_t num = n / 2;
    std::mt19937 mt(1234);
    std::vector<size_t> indices(n);
    std::iota(indices.begin(), indices.end(), 0);
    for (size_t i = 0; i < num; ++i) {
        std::uniform_int_distribution<size_t> dist(i, n - 1);
        std::swap(indices[i], indices[dist(mt)]);
    }
    std::vector<uint32_t> want(indices.begin(), indices.begin() + (std::ptrdiff_t)num);
    std::sort(want.begin(), want.end());
    both_ways(n, mask, want, [&](PointCloudShared& in, PointCloudShared& out) {
        alg::filter::PreprocessFilter filter(*Q);
        filter.random_sampling(in, out, num);
    });
}

// |cos| between the point and its normal inside [cos(max), cos(min)]; a zero normal is removed. The normals win over the covariances
static void angle_incidence_rows(size_t n, unsigned mask) {
    if (!(mask & (COV | NRM))) return;
    const auto want = kept_by(n, [&](size_t i) {
        if ((mask & NRM) && i == 0) return false;
        const double s = 1.25 + double(i), x = i % 2 ? s : double(0.01f * float(s));
        const double c = x / std::sqrt(x * x + s * s);
        return c >= std::cos(double(kMaxAngle)) && c <= std::cos(double(kMinAngle));
    });
    CHECK(n < 2 || (want.size() == n / 2 && want[0] == 1));  // the odd points, as the cloud is made
    alg::filter::PreprocessFilter filter(*Q);
    both_ways(n, mask, want, [&](PointCloudShared& in, PointCloudShared& out) { filter.angle_incidence_filter(in, out, kMinAngle, kMaxAngle); });
}

// OutlierRemoval::radius: the kept set is the filter's own flags; the attributes the cloud lacks and its times are not touched
static void outlier_radius_rows(size_t n, unsigned mask) {
    PointCloudShared cloud(*Q, tagged_cloud(n, mask));
    const void* const before[5] = {cloud.covs.get(), cloud.normals.get(), cloud.rgb.get(), cloud.intensities.get(), cloud.timestamp_offsets.get()};
    const auto tree = alg::knn::KDTree::build(*Q, cloud);
    alg::filter::OutlierRemoval filter(*Q);
    filter.radius(cloud, *tree, 1, 5.0f);  // (squared distance to the nearest other point: about 4 between even points, 8 between odd ones)
    const auto& flags = filter.get_flags().host();
    CHECK(flags.size() == n);
    const auto want = kept_by(flags.size(), [&](size_t i) { return flags[i] != 0; });
    CHECK(n < 65 || (want.size() > 0 && want.size() < n));
    check_rows(cloud, mask, want);
    CHECK(times_are(cloud, kStart, kEnd));
    const void* const after[5] = {cloud.covs.get(), cloud.normals.get(), cloud.rgb.get(), cloud.intensities.get(), cloud.timestamp_offsets.get()};
    for (int a = 0; a < 5; ++a) CHECK((mask >> a & 1u) || after[a] == before[a]);
}

// erase(a, b): with time stamps the end time becomes start + the largest offset left (both 0 when none is left), else the times stay
static void erase_rows(size_t n, unsigned mask) {
    const std::pair<size_t, size_t> cuts[] = {{n / 4, 3 * n / 4}, {0, n}};
    for (const auto& [a, b] : cuts) {
        PointCloudShared cloud(*Q, tagged_cloud(n, mask));
        cloud.erase(a, b);
        const auto want = kept_by(n, [a = a, b = b](size_t i) { return i < a || i >= b; });
        check_rows(cloud, mask, want);
        if (!(mask & STAMPS)) CHECK(times_are(cloud, kStart, kEnd));
        else if (want.empty()) CHECK(times_are(cloud, 0.0, 0.0));
        else CHECK(times_are(cloud, kStart, kStart + double(want.back())));
    }
}

// extend: an attribute survives when both clouds have it; the time stamps of two non-empty clouds do not (the offsets are left
// as they were, no longer one per point), and the times stay. An empty cloud takes the other's points, time stamps and times only.
static void extend_rows(size_t n, unsigned mask) {
    const size_t m = 65;
    for (unsigned other_mask : {mask, unsigned(ALL)}) {
        PointCloudShared cloud(*Q, tagged_cloud(n, mask));
        const PointCloudShared other(*Q, tagged_cloud(m, other_mask));
        cloud.extend(other);
        std::vector<uint32_t> want(n + m);
        std::iota(want.begin(), want.begin() + (std::ptrdiff_t)n, 0u);
        std::iota(want.begin() + (std::ptrdiff_t)n, want.end(), 0u);
        CHECK(cloud.timestamp_offsets->size() == ((mask & STAMPS) ? n : 0));
        cloud.timestamp_offsets->clear();
        check_rows(cloud, mask & ~unsigned(STAMPS), want);
        CHECK(times_are(cloud, kStart, kEnd));
    }
    PointCloudShared empty(*Q);
    PointCloudShared other(*Q, tagged_cloud(n, mask));
    other.start_time_ms = 7.0;
    empty += other;
    std::vector<uint32_t> all(n);
    std::iota(all.begin(), all.end(), 0u);
    check_rows(empty, mask & STAMPS, all);
    CHECK((mask & STAMPS) ? times_are(empty, 7.0, kEnd) : times_are(empty, 0.0, 0.0));
}

// the copy constructor: every row and the times, in containers of its own
static void copy_rows(size_t n, unsigned mask) {
    const PointCloudShared cloud(*Q, tagged_cloud(n, mask));
    const PointCloudShared copy(cloud);
    std::vector<uint32_t> all(n);
    std::iota(all.begin(), all.end(), 0u);
    check_rows(copy, mask, all);
    check_rows(cloud, mask, all);
    CHECK(times_are(copy, kStart, kEnd));
    CHECK(copy.points != cloud.points && copy.covs != cloud.covs && copy.normals != cloud.normals && copy.rgb != cloud.rgb &&
          copy.intensities != cloud.intensities && copy.timestamp_offsets != cloud.timestamp_offsets);
}

template <class V>
static std::vector<unsigned char> bytes_of(const V& v) {
    const auto& h = v.host();
    const unsigned char* p = reinterpret_cast<const unsigned char*>(h.data());
    return std::vector<unsigned char>(p, p + h.size() * sizeof(typename V::value_type));
}
// One point per voxel and min_voxel_count 1: the output is a permutation of the input, without covariances and normals; the times
// are the cloud's only when it has time stamps; in place gives the bytes of out of place. make(): a fresh grid for every call
template <class MakeGrid>
static void downsampled_rows(size_t n, unsigned mask, MakeGrid&& make) {
    const PointCloudCPU cpu = tagged_cloud(n, mask);
    const PointCloudShared source(*Q, cpu);
    PointCloudShared output = used_output();
    make().downsampling(source, output);
    CHECK(output.size() == n);
    std::vector<uint32_t> order;
    for (const auto& p : output.points->host()) order.push_back(uint32_t(std::lround(tag_of(p))));
    std::vector<uint32_t> sorted = order, all(n);
    std::sort(sorted.begin(), sorted.end());
    std::iota(all.begin(), all.end(), 0u);
    CHECK(sorted == all);
    check_rows(output, mask & (RGB | INTEN | STAMPS), order, /*exact_points=*/false);
    CHECK((mask & STAMPS) ? times_are(output, kStart, kEnd) : times_are(output, 1.0, 2.0));
    PointCloudShared data(*Q, cpu);
    make().downsampling(data, data);
    check_rows(data, mask & (RGB | INTEN | STAMPS), order, /*exact_points=*/false);
    CHECK(times_are(data, kStart, kEnd));
    CHECK(bytes_of(*data.points) == bytes_of(*output.points) && bytes_of(*data.rgb) == bytes_of(*output.rgb) &&
          bytes_of(*data.intensities) == bytes_of(*output.intensities) &&
          bytes_of(*data.timestamp_offsets) == bytes_of(*output.timestamp_offsets));
}
// voxels of 0.5: the points are at least 1 apart in y, at y = 1.25 + i in the middle of a voxel
static void voxel_grid_rows(size_t n, unsigned mask) {
    downsampled_rows(n, mask, [] {
        alg::filter::VoxelGrid grid(*Q, 0.5f);
        grid.set_min_voxel_count(1);
        return grid;
    });
}
// 0.5 in distance, 0.1 rad in both angles: odd and even points are 0.78 rad apart in azimuth, points of one kind 2 or more in distance
static void polar_grid_rows(size_t n, unsigned mask) {
    downsampled_rows(n, mask, [] {
        alg::filter::PolarGrid grid(*Q, 0.5f, 0.1f, 0.1f);
        grid.set_min_voxel_count(1);
        return grid;
    });
}

int main() {
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(box_filter_rows);
    RUN(random_sampling_rows);
    RUN(angle_incidence_rows);
    RUN(outlier_radius_rows);
    RUN(erase_rows);
    RUN(extend_rows);
    RUN(copy_rows);
    RUN(voxel_grid_rows);
    RUN(polar_grid_rows);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
