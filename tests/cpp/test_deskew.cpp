// C++ tests of the constant-velocity deskew and the pipeline's velocity update, included through the reference's paths only:
// the reference's RelativePoseDeskewTest cases (cpp/tests/test_relative_pose_deskew.cpp, restated), RegistrationPipelineTest's
// velocity-update cases (cpp/tests/test_registration_pipeline.cpp:221-358, :510-540, restated), the in-place call that pins the
// documented deviation, and an end-to-end run on a skewed scan. Built and run by tests/test_gpu_deskew.py on a GPU box; exit
// code 0 = all checks passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "sycl_points/algorithms/deskew/relative_pose_deskew.hpp"
#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/knn/knn.hpp"
#include "sycl_points/algorithms/registration/pipeline/velocity_update.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"
#include "sycl_points/algorithms/registration/registration_pipeline.hpp"

using namespace sycl_points;
namespace alg = sycl_points::algorithms;
namespace reg = sycl_points::algorithms::registration;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); } while (0)

static sycl_utils::DeviceQueue* Q = nullptr;

// ------------------------------------------------------------------------------------------------ float64 pose algebra
struct Pose64 {
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    double t[3] = {0, 0, 0};
};
static Pose64 exp64(const double a[6]) {
    Pose64 o;
    const double th = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double O[3][3] = {{0, -a[2], a[1]}, {a[2], 0, -a[0]}, {-a[1], a[0], 0}};
    double O2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    const double A = th < 1e-9 ? 1.0 : std::sin(th) / th, B = th < 1e-9 ? 0.5 : (1 - std::cos(th)) / (th * th),
                 Cc = th < 1e-9 ? 1.0 / 6 : (th - std::sin(th)) / (th * th * th);
    for (int i = 0; i < 3; ++i) {
        o.t[i] = 0;
        for (int j = 0; j < 3; ++j) {
            o.R[i][j] = (i == j) + A * O[i][j] + B * O2[i][j];
            o.t[i] += ((i == j) + B * O[i][j] + Cc * O2[i][j]) * a[3 + j];
        }
    }
    return o;
}
static Pose64 mul64(const Pose64& a, const Pose64& b) {
    Pose64 o;
    for (int i = 0; i < 3; ++i) {
        o.t[i] = a.t[i];
        for (int j = 0; j < 3; ++j) {
            o.R[i][j] = a.R[i][0] * b.R[0][j] + a.R[i][1] * b.R[1][j] + a.R[i][2] * b.R[2][j];
            o.t[i] += a.R[i][j] * b.t[j];
        }
    }
    return o;
}
static Pose64 inv64(const Pose64& a) {
    Pose64 o;
    for (int i = 0; i < 3; ++i) {
        o.t[i] = 0;
        for (int j = 0; j < 3; ++j) {
            o.R[i][j] = a.R[j][i];
            o.t[i] -= a.R[j][i] * a.t[j];
        }
    }
    return o;
}
static Eigen::Isometry3f to_iso(const Pose64& p) {
    TransformMatrix m = TransformMatrix::Identity();
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m(i, j) = float(p.R[i][j]);
        m(i, 3) = float(p.t[i]);
    }
    return Eigen::Isometry3f(m);
}

static bool same_bytes(const void* a, const void* b, size_t n) { return std::memcmp(a, b, n) == 0; }

// ------------------------------------------------------------------------------------------------ RelativePoseDeskewTest
// DeskewsPointsWithConstantVelocity (:13-76)
static void deskews_points_with_constant_velocity() {
    const Pose64 start;
    Pose64 end;
    end.R[0][0] = 0; end.R[0][1] = -1; end.R[1][0] = 1; end.R[1][1] = 0;  // 90 degrees about z
    end.t[0] = 1.0;
    const Eigen::Isometry3f start_pose = to_iso(start), end_pose = to_iso(end);
    float twist[6];
    sp_relative_twist_host(start_pose.matrix().data(), end_pose.matrix().data(), twist);
    const double W[3] = {1, 1, 0}, N[3] = {0, 0, 1}, Cd[3] = {0.01, 0.02, 0.03};
    PointCloudShared cloud(*Q);
    cloud.start_time_ms = 0.0;
    for (double ts : {0.0, 0.5, 1.0}) {
        double a[6];
        for (int k = 0; k < 6; ++k) a[k] = double(twist[k]) * ts;
        const Pose64 pi = inv64(mul64(start, exp64(a)));
        PointType p(0, 0, 0, 1);
        Normal n(0, 0, 0, 0);
        Covariance C = Covariance::Zero();
        for (int i = 0; i < 3; ++i) {
            p[i] = float(pi.R[i][0] * W[0] + pi.R[i][1] * W[1] + pi.R[i][2] * W[2] + pi.t[i]);
            n[i] = float(pi.R[i][0] * N[0] + pi.R[i][1] * N[1] + pi.R[i][2] * N[2]);
            for (int j = 0; j < 3; ++j) C(i, j) = float(pi.R[i][0] * Cd[0] * pi.R[j][0] + pi.R[i][1] * Cd[1] * pi.R[j][1] + pi.R[i][2] * Cd[2] * pi.R[j][2]);
        }
        cloud.timestamp_offsets->push_back(float(ts * 1e3));
        cloud.points->push_back(p);
        cloud.normals->push_back(n);
        cloud.covs->push_back(C);
    }
    cloud.end_time_ms = 1e3;
    CHECK(cloud.has_timestamps() && cloud.has_normal() && cloud.has_cov());
    PointCloudShared deskewed(*Q);
    CHECK(alg::deskew::deskew_point_cloud_constant_velocity(cloud, deskewed, start_pose, end_pose));
    CHECK(deskewed.size() == 3);
    for (size_t i = 0; i < deskewed.size(); ++i) {
        const auto p = std::as_const(*deskewed.points)[i];
        const auto n = std::as_const(*deskewed.normals)[i];
        const auto C = std::as_const(*deskewed.covs)[i];
        double dp = 0, dn = 0, dc = 0;
        for (int k = 0; k < 3; ++k) {
            dp += (p[k] - W[k]) * (p[k] - W[k]);
            dn += (n[k] - N[k]) * (n[k] - N[k]);
            for (int j = 0; j < 3; ++j) dc += (C(k, j) - (k == j ? Cd[k] : 0.0)) * (C(k, j) - (k == j ? Cd[k] : 0.0));
        }
        CHECK(std::sqrt(dp) <= 1e-5);
        CHECK(std::sqrt(dn) <= 1e-5);
        CHECK(std::sqrt(dc) <= 1e-6);
        CHECK(p[3] == 1.0f && n[3] == 0.0f && C(3, 3) == 0.0f && C(0, 3) == 0.0f && C(3, 0) == 0.0f);
    }
    CHECK(deskewed.start_time_ms == 0.0 && deskewed.end_time_ms == 1e3 && deskewed.has_timestamps());
    CHECK(deskewed.timestamp_offsets.get() != cloud.timestamp_offsets.get());
}

// HandlesNonPositiveScanDuration (:78-95), and the other ways to get `false`
static void handles_non_positive_scan_duration() {
    const Eigen::Isometry3f I = Eigen::Isometry3f::Identity();
    PointCloudShared cloud(*Q);
    cloud.start_time_ms = 0.0;
    cloud.timestamp_offsets->push_back(0);
    cloud.points->push_back(PointType(0, 0, 0, 1));
    cloud.end_time_ms = cloud.start_time_ms;
    PointCloudShared deskewed(*Q);
    CHECK(!alg::deskew::deskew_point_cloud_constant_velocity(cloud, deskewed, I, I));
    CHECK(alg::deskew::deskew_point_cloud_constant_velocity(cloud, deskewed, I, I, 0.1f));  // an explicit duration is enough
    PointCloudShared empty(*Q);
    CHECK(!alg::deskew::deskew_point_cloud_constant_velocity(empty, deskewed, I, I, 0.1f));
    cloud.timestamp_offsets->clear();
    CHECK(!alg::deskew::deskew_point_cloud_constant_velocity(cloud, deskewed, I, I, 0.1f));
}

// The documented deviation: in place returns the rotated normals and covariances (the reference returns zeros there)
static void in_place_returns_rotated_attributes() {
    std::mt19937 mt(5);
    std::uniform_real_distribution<float> u(-20.0f, 20.0f), ut(0.0f, 100.0f);
    PointCloudShared cloud(*Q);
    for (int i = 0; i < 5000; ++i) {
        cloud.points->push_back(PointType(u(mt), u(mt), u(mt), 1.0f));
        cloud.normals->push_back(Normal(0.0f, 0.6f, 0.8f, 0.0f));
        Covariance C = Covariance::Zero();
        C(0, 0) = 0.01f; C(1, 1) = 0.02f; C(2, 2) = 0.03f; C(0, 1) = C(1, 0) = 0.005f;
        cloud.covs->push_back(C);
        cloud.timestamp_offsets->push_back(ut(mt));
    }
    cloud.end_time_ms = 100.0;
    const double a[6] = {0.02, -0.03, 0.05, 1.0, 0.5, -0.2};
    const Eigen::Isometry3f prev = Eigen::Isometry3f::Identity(), cur = to_iso(exp64(a));
    PointCloudShared out(*Q);
    CHECK(alg::deskew::deskew_point_cloud_constant_velocity(cloud, out, prev, cur, 0.1f));
    PointCloudShared inplace(cloud);  // deep copy
    CHECK(alg::deskew::deskew_point_cloud_constant_velocity(inplace, inplace, prev, cur, 0.1f));
    CHECK(same_bytes(inplace.points->host().data(), out.points->host().data(), 5000 * sizeof(PointType)));
    CHECK(same_bytes(inplace.normals->host().data(), out.normals->host().data(), 5000 * sizeof(Normal)));
    CHECK(same_bytes(inplace.covs->host().data(), out.covs->host().data(), 5000 * sizeof(Covariance)));
    size_t nonzero_n = 0, nonzero_c = 0, moved = 0;
    for (size_t i = 0; i < 5000; ++i) {
        const auto n = std::as_const(*inplace.normals)[i];
        const auto C = std::as_const(*inplace.covs)[i];
        nonzero_n += std::fabs(std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) - 1.0f) < 1e-5f;
        nonzero_c += std::fabs(C(0, 0) + C(1, 1) + C(2, 2) - 0.06f) < 1e-6f;  // the trace is kept by a rotation
        moved += !(n == std::as_const(*cloud.normals)[i]);
    }
    CHECK(nonzero_n == 5000 && nonzero_c == 5000 && moved > 4900);
    CHECK(inplace.has_timestamps() && inplace.size() == 5000);
}

// The output side of the call, which the IMU deskew shares: out of place, an output cloud that held other rows and attributes
// ends up with the input's rgb, stamps and times and without the attributes the input does not have; in place leaves them alone
static void output_takes_the_attributes_the_deskew_does_not_touch() {
    PointCloudShared cloud(*Q);
    for (int i = 0; i < 8; ++i) {
        cloud.points->push_back(PointType(float(i), 1.0f, 2.0f, 1.0f));
        cloud.rgb->push_back(RGBType(0.125f * float(i), 0.5f, 0.25f, 1.0f));
        cloud.timestamp_offsets->push_back(12.5f * float(i));
    }
    cloud.start_time_ms = 1000.0;
    cloud.end_time_ms = 1100.0;
    PointCloudShared out(*Q);
    for (int i = 0; i < 5; ++i) {
        out.points->push_back(PointType(0, 0, 0, 1));
        out.normals->push_back(Normal(0, 0, 1, 0));
        out.covs->push_back(Covariance::Zero());
        out.rgb->push_back(RGBType(1, 1, 1, 1));
        out.intensities->push_back(7.0f);
    }
    const std::vector<RGBType, Eigen::aligned_allocator<RGBType>> rgb(cloud.rgb->host().begin(), cloud.rgb->host().end());
    const std::vector<float> stamps(cloud.timestamp_offsets->host().begin(), cloud.timestamp_offsets->host().end());
    auto untouched = [&](const PointCloudShared& c) {
        return c.size() == 8 && c.normals->empty() && c.covs->empty() && c.intensities->empty() && c.rgb->size() == 8 &&
               c.timestamp_offsets->size() == 8 && std::memcmp(c.rgb->host().data(), rgb.data(), 8 * sizeof(RGBType)) == 0 &&
               std::memcmp(c.timestamp_offsets->host().data(), stamps.data(), 8 * sizeof(float)) == 0 && c.start_time_ms == 1000.0 &&
               c.end_time_ms == 1100.0;
    };
    const double a[6] = {0.02, -0.03, 0.05, 1.0, 0.5, -0.2};
    const Eigen::Isometry3f prev = Eigen::Isometry3f::Identity(), cur = to_iso(exp64(a));
    CHECK(alg::deskew::deskew_point_cloud_constant_velocity(cloud, out, prev, cur, 0.1f));
    CHECK(untouched(out));
    CHECK(alg::deskew::deskew_point_cloud_constant_velocity(cloud, cloud, prev, cur, 0.1f));
    CHECK(untouched(cloud));
    CHECK(same_bytes(cloud.points->host().data(), out.points->host().data(), 8 * sizeof(PointType)));
}

// ------------------------------------------------------------------------------------------------ RegistrationPipelineTest
namespace {
class DummyKNN : public alg::knn::KNNBase {  // test_registration_pipeline.cpp:16-23
public:
    sycl_utils::events knn_search_async(const PointCloudShared&, const size_t, alg::knn::KNNResult&,
                                        const std::vector<sycl_utils::event>& = std::vector<sycl_utils::event>(),
                                        const TransformMatrix& = TransformMatrix::Identity()) const override {
        return sycl_utils::events();
    }
};
class CountingNearestKNN : public alg::knn::KNNBase {  // test_registration_pipeline.cpp:25-61
public:
    mutable size_t call_count = 0;
    sycl_utils::events knn_search_async(const PointCloudShared& queries, const size_t k, alg::knn::KNNResult& result,
                                        const std::vector<sycl_utils::event>& = std::vector<sycl_utils::event>(),
                                        const TransformMatrix& T = TransformMatrix::Identity()) const override {
        ++call_count;
        result.allocate(queries.queue, queries.size(), k);
        std::vector<int32_t> idx(queries.size() * k, -1);
        std::vector<float> dist(queries.size() * k, std::numeric_limits<float>::max());
        for (size_t i = 0; i < queries.size(); ++i) {
            const PointType q = std::as_const(*queries.points)[i];
            float x[3];
            for (int r = 0; r < 3; ++r) x[r] = T(r, 0) * q[0] + T(r, 1) * q[1] + T(r, 2) * q[2] + T(r, 3) * q[3];
            for (size_t j = 0; j < target_->size(); ++j) {
                const PointType t = std::as_const(*target_->points)[j];
                const float d = (x[0] - t[0]) * (x[0] - t[0]) + (x[1] - t[1]) * (x[1] - t[1]) + (x[2] - t[2]) * (x[2] - t[2]);
                if (d < dist[i * k]) { dist[i * k] = d; idx[i * k] = int32_t(j); }
            }
        }
        result.indices->assign(idx.data(), idx.size());
        result.distances->assign(dist.data(), dist.size());
        return sycl_utils::events();
    }
    void set_target(const PointCloudShared& target) { target_ = &target; }

private:
    const PointCloudShared* target_ = nullptr;
};
PointCloudShared make_cloud(size_t size) {  // test_registration_pipeline.cpp:63-78
    PointCloudShared cloud(*Q);
    cloud.points->resize(size);
    cloud.intensities->resize(size);
    cloud.timestamp_offsets->resize(size);
    for (size_t i = 0; i < size; ++i) {
        cloud.points->data()[i] = PointType(static_cast<float>(i), static_cast<float>(i + 1), static_cast<float>(i + 2), 1.0f);
        cloud.intensities->data()[i] = static_cast<float>(i);
        cloud.timestamp_offsets->data()[i] = static_cast<float>(i) * 0.1f;
    }
    cloud.start_time_ms = 1.0;
    cloud.end_time_ms = 2.0;
    return cloud;
}
reg::RegistrationResult translated(float x, size_t inlier) {
    reg::RegistrationResult result;
    result.T.matrix()(0, 3) = x;
    result.inlier = static_cast<uint32_t>(inlier);
    return result;
}
}  // namespace

static void accessors_return_null_before_align() {  // :221-234
    auto nothing = [](const PointCloudShared&, const PointCloudShared&, const alg::knn::KNNBase&, const TransformMatrix&,
                      const reg::Registration::ExecutionOptions&) { return reg::RegistrationResult{}; };
    reg::RegistrationPipeline pipeline(nothing);
    CHECK(pipeline.get_registration_input_point_cloud() == nullptr);
    CHECK(pipeline.get_deskewed_point_cloud() == nullptr);
    reg::pipeline::VelocityUpdateAligner velocity_pipeline(nothing, 1, false);
    CHECK(velocity_pipeline.get_deskewed_point_cloud() == nullptr);
    reg::RegistrationPipelineParams params;
    CHECK(!params.velocity_update.enable && params.velocity_update.iter == 1);  // registration_pipeline_params.hpp
    params.velocity_update.enable = true;
    reg::RegistrationPipeline with_stage(nothing, params);
    CHECK(with_stage.get_deskewed_point_cloud() == nullptr);
}

static void velocity_update_aligner_exposes_most_recent_deskewed_point_cloud() {  // :236-265
    const auto source = make_cloud(4);
    const auto target = make_cloud(3);
    DummyKNN knn;
    size_t calls = 0;
    auto aligner = [&](const PointCloudShared& s, const PointCloudShared&, const alg::knn::KNNBase&, const TransformMatrix&,
                       const reg::Registration::ExecutionOptions&) { ++calls; return translated(1.0f, s.size()); };
    reg::pipeline::VelocityUpdateAligner pipeline(aligner, 1, false);
    reg::Registration::ExecutionOptions options;
    options.dt = 1.0f;
    options.prev_pose = TransformMatrix::Identity();
    pipeline.align(source, target, knn, TransformMatrix::Identity(), options);
    const auto deskewed = pipeline.get_deskewed_point_cloud();
    CHECK(deskewed != nullptr && calls == 1);
    CHECK(deskewed->size() == source.size());
    CHECK(deskewed->has_timestamps() && deskewed->has_intensity());
    CHECK(deskewed->points.get() != source.points.get());
    CHECK(deskewed->intensities.get() != source.intensities.get());
    CHECK(deskewed->timestamp_offsets.get() != source.timestamp_offsets.get());
    CHECK(deskewed->start_time_ms == 1.0 && deskewed->end_time_ms == 2.0);
    // iter = 0 still makes one round; iter = 3 makes three, each from the previous round's pose; an empty source none
    reg::pipeline::VelocityUpdateAligner zero(aligner, 0, false), three(aligner, 3, false);
    calls = 0;
    zero.align(source, target, knn, TransformMatrix::Identity(), options);
    CHECK(calls == 1);
    three.align(source, target, knn, TransformMatrix::Identity(), options);
    CHECK(calls == 4);
    PointCloudShared empty(*Q);
    TransformMatrix guess = TransformMatrix::Identity();
    guess(1, 3) = 2.0f;
    const auto r = three.align(empty, target, knn, guess, options);
    CHECK(calls == 4 && r.T.matrix() == guess);
}

static void velocity_update_aligner_falls_back_without_timestamps() {  // :267-302
    auto source = make_cloud(4);
    source.timestamp_offsets->clear();
    source.start_time_ms = 0.0;
    source.end_time_ms = 0.0;
    const auto target = make_cloud(3);
    DummyKNN knn;
    bool aligned_source_has_timestamps = true;
    size_t aligned_source_size = 0, calls = 0;
    auto aligner = [&](const PointCloudShared& s, const PointCloudShared&, const alg::knn::KNNBase&, const TransformMatrix&,
                       const reg::Registration::ExecutionOptions&) {
        ++calls;
        aligned_source_has_timestamps = s.has_timestamps();
        aligned_source_size = s.size();
        return translated(0.0f, s.size());
    };
    reg::pipeline::VelocityUpdateAligner pipeline(aligner, 2, false);
    reg::Registration::ExecutionOptions options;
    options.dt = 1.0f;
    options.prev_pose = TransformMatrix::Identity();
    const auto result = pipeline.align(source, target, knn, TransformMatrix::Identity(), options);
    CHECK(result.inlier == source.size() && calls == 1);
    CHECK(aligned_source_size == source.size());
    CHECK(!aligned_source_has_timestamps);
    const auto deskewed = pipeline.get_deskewed_point_cloud();
    CHECK(deskewed != nullptr);
    CHECK(deskewed->size() == source.size());
    CHECK(!deskewed->has_timestamps());
    CHECK(deskewed->points.get() == source.points.get());  // forwarded by shallow assignment
}

static void registration_pipeline_exposes_deskewed_point_cloud() {  // :304-334
    reg::RegistrationPipelineParams params;
    params.velocity_update.enable = true;
    params.velocity_update.iter = 1;
    auto aligner = [&](const PointCloudShared& s, const PointCloudShared&, const alg::knn::KNNBase&, const TransformMatrix&,
                       const reg::Registration::ExecutionOptions&) { return translated(0.5f, s.size()); };
    reg::RegistrationPipeline pipeline(aligner, params);
    reg::Registration::ExecutionOptions options;
    options.dt = 1.0f;
    options.prev_pose = TransformMatrix::Identity();
    DummyKNN knn;
    const auto source = make_cloud(5);
    pipeline.align(source, make_cloud(3), knn, TransformMatrix::Identity(), options);
    const auto deskewed = pipeline.get_deskewed_point_cloud();
    CHECK(deskewed != nullptr);
    CHECK(deskewed->size() == 5);
    CHECK(deskewed->points.get() != source.points.get());
    CHECK(deskewed->intensities.get() != source.intensities.get());
    CHECK(deskewed->timestamp_offsets.get() != source.timestamp_offsets.get());
}

static void deskewed_accessor_falls_back_to_registration_input_without_velocity_update() {  // :336-358
    reg::RegistrationPipelineParams params;
    params.random_sampling.enable = true;
    params.random_sampling.num = 2;
    auto aligner = [&](const PointCloudShared& s, const PointCloudShared&, const alg::knn::KNNBase&, const TransformMatrix&,
                       const reg::Registration::ExecutionOptions&) { return translated(0.0f, s.size()); };
    reg::RegistrationPipeline pipeline(aligner, params);
    DummyKNN knn;
    pipeline.align(make_cloud(5), make_cloud(3), knn);
    CHECK(pipeline.get_deskewed_point_cloud().get() == pipeline.get_registration_input_point_cloud());
    CHECK(pipeline.get_deskewed_point_cloud() != nullptr);
    CHECK(pipeline.get_deskewed_point_cloud()->size() == 2);
}

static void pipeline_lazy_weights_match_deskewed_point_cloud_size() {  // :510-540
    reg::RegistrationPipelineParams params;
    params.registration.reg_type = reg::RegType::POINT_TO_POINT;
    params.registration.robust.type = alg::robust::RobustLossType::NONE;
    params.registration.max_iterations = 1;
    params.registration.max_correspondence_distance = 1.5f;
    params.velocity_update.enable = true;
    params.velocity_update.iter = 1;
    reg::RegistrationPipeline pipeline(*Q, params);
    PointCloudShared source(*Q), target(*Q);
    const float sx[3] = {0.0f, 1.0f, 5.0f}, st[3] = {0.0f, 0.5f, 1.0f};
    for (int i = 0; i < 3; ++i) {
        source.points->push_back(PointType(sx[i], 0.0f, 0.0f, 1.0f));
        source.timestamp_offsets->push_back(st[i]);
    }
    source.start_time_ms = 0.0;
    source.end_time_ms = 1.0;
    target.points->push_back(PointType(0.0f, 0.0f, 0.0f, 1.0f));
    target.points->push_back(PointType(1.0f, 0.0f, 0.0f, 1.0f));
    CountingNearestKNN knn;
    knn.set_target(target);
    reg::Registration::ExecutionOptions options;
    options.dt = 1.0f;
    options.prev_pose = TransformMatrix::Identity();
    pipeline.align(source, target, knn, TransformMatrix::Identity(), options);
    const auto deskewed = pipeline.get_deskewed_point_cloud();
    CHECK(deskewed != nullptr && knn.call_count > 0);
    shared_vector<float> weights(*Q);
    pipeline.compute_icp_robust_weights(target, knn, TransformMatrix::Identity(), params.registration.robust.default_scale, weights);
    CHECK(deskewed != nullptr && weights.size() == deskewed->size() && weights.size() == 3);
}

// ------------------------------------------------------------------------------------------------ end to end
// A room seen from a sensor that moves at constant body velocity: the previous scan started at pose P0 = identity, this scan
// starts at T_gt = exp(xi) and the sensor keeps moving while it is taken: a world point sampled at tau in [0, 1] of the scan
// period is observed from T_gt * exp(xi * tau). The target is the room in the world frame.
struct Scene {
    PointCloudShared target, source;
    Eigen::Isometry3f T_gt;
    TransformMatrix guess;
    Scene() : target(*Q), source(*Q) {}
};
static void make_scene(Scene& s, size_t n) {
    std::mt19937_64 mt(1234);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const double xi[6] = {0.01, -0.015, 0.05, 1.4, 0.5, -0.1};  // "driving": 0.05 rad and 1.5 m per scan
    const Pose64 Tgt = exp64(xi);
    PointCloudCPU tc, sc;
    for (size_t i = 0; i < n; ++i) {
        double W[3];
        const double r = u(mt), a = u(mt) * 40.0 - 20.0, b = u(mt);
        if (r < 0.5) { W[0] = a; W[1] = b * 40.0 - 20.0; W[2] = -1.5 + 0.01 * (u(mt) - 0.5); }          // ground
        else if (r < 0.625) { W[0] = a; W[1] = 20.0; W[2] = -1.5 + 6.0 * b; }                            // four walls
        else if (r < 0.75) { W[0] = a; W[1] = -20.0; W[2] = -1.5 + 6.0 * b; }
        else if (r < 0.875) { W[0] = 20.0; W[1] = a; W[2] = -1.5 + 6.0 * b; }
        else { W[0] = -20.0; W[1] = a; W[2] = -1.5 + 6.0 * b; }
        if (r >= 0.5 && std::fmod(std::fabs(a), 8.0) < 2.0) {  // pilasters: structure along the walls
            if (std::fabs(W[0]) == 20.0) W[0] *= 0.975; else W[1] *= 0.975;
        }
        tc.points->push_back(PointType(float(W[0]), float(W[1]), float(W[2]), 1.0f));
        const double tau = u(mt);
        double at[6];
        for (int k = 0; k < 6; ++k) at[k] = xi[k] * tau;
        const Pose64 pi = inv64(mul64(Tgt, exp64(at)));
        sc.points->push_back(PointType(float(pi.R[0][0] * W[0] + pi.R[0][1] * W[1] + pi.R[0][2] * W[2] + pi.t[0]),
                                       float(pi.R[1][0] * W[0] + pi.R[1][1] * W[1] + pi.R[1][2] * W[2] + pi.t[1]),
                                       float(pi.R[2][0] * W[0] + pi.R[2][1] * W[1] + pi.R[2][2] * W[2] + pi.t[2]), 1.0f));
        sc.timestamp_offsets->push_back(float(tau * 100.0));
    }
    sc.start_time_ms = 0.0;
    sc.end_time_ms = 100.0;
    s.target = PointCloudShared(*Q, tc);
    s.source = PointCloudShared(*Q, sc);
    s.T_gt = to_iso(Tgt);
    double xg[6];
    for (int k = 0; k < 6; ++k) xg[k] = 0.8 * xi[k];  // the motion model's prediction: the previous motion, 20 % off
    s.guess = to_iso(exp64(xg)).matrix();
    const auto tgrid = alg::knn::GridKNN::build(*Q, s.target);
    alg::covariance::estimate_async(*tgrid, s.target, 20).wait_and_throw();
    const auto sgrid = alg::knn::GridKNN::build(*Q, s.source);
    alg::covariance::estimate_async(*sgrid, s.source, 20).wait_and_throw();
}
static bool same_result(const reg::RegistrationResult& a, const reg::RegistrationResult& b) {
    return a.T.matrix() == b.T.matrix() && a.H == b.H && a.b == b.b && same_bytes(&a.error, &b.error, 4) && a.inlier == b.inlier &&
           a.iterations == b.iterations && a.converged == b.converged;
}
static float pose_error(const Eigen::Isometry3f& T_gt, const Eigen::Isometry3f& T, float* angle, float* dist) {
    float tw[6];
    sp_relative_twist_host(T_gt.matrix().data(), T.matrix().data(), tw);
    *angle = std::sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]);
    *dist = std::sqrt(tw[3] * tw[3] + tw[4] * tw[4] + tw[5] * tw[5]);
    return std::sqrt(*angle * *angle + *dist * *dist);
}

static void end_to_end() {
    Scene s;
    const size_t n = 100000;
    make_scene(s, n);
    const auto grid = alg::knn::GridKNN::build(*Q, s.target);
    reg::RegistrationPipelineParams params;
    params.registration.max_iterations = 20;
    params.random_sampling.enable = false;
    reg::Registration::ExecutionOptions options;
    options.dt = 0.1f;
    options.prev_pose = TransformMatrix::Identity();

    // 1. iter = 1: the deskewed cloud is sp_deskew_constant_velocity applied with (prev_pose, initial_guess), bit for bit, and the
    //    result is Registration::align on that cloud, bit for bit
    {
        auto p1 = params;
        p1.velocity_update.enable = true;
        p1.velocity_update.iter = 1;
        reg::RegistrationPipeline pipeline(*Q, p1);
        const auto r = pipeline.align(s.source, s.target, *grid, s.guess, options);
        const auto deskewed = pipeline.get_deskewed_point_cloud();
        CHECK(deskewed != nullptr && deskewed->size() == n && deskewed->has_cov() && deskewed->has_timestamps());
        float tw[6];
        sp_relative_twist_host(options.prev_pose.data(), s.guess.data(), tw);
        float *pd = nullptr, *cd = nullptr;
        CHECK(hipMalloc(&pd, n * 16) == hipSuccess && hipMalloc(&cd, n * 64) == hipSuccess);
        CHECK(sp_deskew_constant_velocity(s.source.points_device(), s.source.covs_device(), nullptr,
                                          s.source.timestamp_offsets->device_data(), n, tw, options.dt, pd, cd, nullptr,
                                          Q->stream()) == SP_OK);
        std::vector<float> ph(n * 4), ch(n * 16);
        CHECK(hipMemcpy(ph.data(), pd, n * 16, hipMemcpyDeviceToHost) == hipSuccess);
        CHECK(hipMemcpy(ch.data(), cd, n * 64, hipMemcpyDeviceToHost) == hipSuccess);
        (void)hipFree(pd);
        (void)hipFree(cd);
        CHECK(same_bytes(ph.data(), deskewed->points->host().data(), n * 16));
        CHECK(same_bytes(ch.data(), deskewed->covs->host().data(), n * 64));
        CHECK(!same_bytes(ph.data(), s.source.points->host().data(), n * 16));
        reg::Registration direct(*Q, params.registration);
        const auto rd = direct.align(*deskewed, s.target, *grid, s.guess, options);
        CHECK(same_result(r, rd));
        CHECK(r.inlier > n / 2);
    }
    // 2. enable = false: the pipeline is what it was — Registration::align on the input, and with the annealing schedule the
    //    RobustAligner that talks to the backend (all levels in one launch)
    reg::RegistrationResult r_off;
    {
        reg::RegistrationPipeline pipeline(*Q, params);
        r_off = pipeline.align(s.source, s.target, *grid, s.guess, options);
        CHECK(pipeline.get_deskewed_point_cloud().get() == pipeline.get_registration_input_point_cloud());
        CHECK(pipeline.get_deskewed_point_cloud()->points.get() == s.source.points.get());
        reg::Registration direct(*Q, params.registration);
        CHECK(same_result(r_off, direct.align(s.source, s.target, *grid, s.guess, options)));
        auto pr = params;
        pr.registration.robust.type = alg::robust::RobustLossType::GEMAN_MCCLURE;
        pr.robust.auto_scale = true;
        pr.robust.auto_scaling_iter = 3;
        reg::RegistrationPipeline annealed(*Q, pr);
        const auto ra = annealed.align(s.source, s.target, *grid, s.guess, options);
        reg::pipeline::RobustAligner robust(std::make_shared<reg::Registration>(*Q, pr.registration), pr);
        CHECK(same_result(ra, robust.align(s.source, s.target, *grid, s.guess, options)));
    }
    // 3. iter = 2 lands closer to the ground truth than the same pipeline with the stage off, on the same skewed source
    {
        auto p2 = params;
        p2.velocity_update.enable = true;
        p2.velocity_update.iter = 2;
        reg::RegistrationPipeline pipeline(*Q, p2);
        const auto r_on = pipeline.align(s.source, s.target, *grid, s.guess, options);
        float a_on, d_on, a_off, d_off;
        const float e_on = pose_error(s.T_gt, r_on.T, &a_on, &d_on), e_off = pose_error(s.T_gt, r_off.T, &a_off, &d_off);
        std::printf("  pose error against the ground truth (norm of se3_log(T_gt^-1 T)):\n"
                    "    velocity update off        : %.6f  (angle %.6f rad, distance %.6f m)\n"
                    "    velocity update on, iter 2 : %.6f  (angle %.6f rad, distance %.6f m)\n",
                    e_off, a_off, d_off, e_on, a_on, d_on);
        CHECK(e_on < e_off);
        // the same with the annealing schedule around it: RobustAligner -> VelocityUpdateAligner -> Registration::align
        p2.registration.robust.type = alg::robust::RobustLossType::GEMAN_MCCLURE;
        p2.robust.auto_scale = true;
        p2.robust.auto_scaling_iter = 2;
        reg::RegistrationPipeline nested(*Q, p2);
        const auto r_nested = nested.align(s.source, s.target, *grid, s.guess, options);
        float a_n, d_n;
        const float e_n = pose_error(s.T_gt, r_nested.T, &a_n, &d_n);
        std::printf("    ... inside 2 robust levels : %.6f  (angle %.6f rad, distance %.6f m)\n", e_n, a_n, d_n);
        CHECK(e_n < e_off);
        CHECK(nested.get_deskewed_point_cloud() != nullptr && nested.get_deskewed_point_cloud()->size() == n);
    }
}

int main() {
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(deskews_points_with_constant_velocity);
    RUN(handles_non_positive_scan_duration);
    RUN(in_place_returns_rotated_attributes);
    RUN(output_takes_the_attributes_the_deskew_does_not_touch);
    RUN(accessors_return_null_before_align);
    RUN(velocity_update_aligner_exposes_most_recent_deskewed_point_cloud);
    RUN(velocity_update_aligner_falls_back_without_timestamps);
    RUN(registration_pipeline_exposes_deskewed_point_cloud);
    RUN(deskewed_accessor_falls_back_to_registration_input_without_velocity_update);
    RUN(pipeline_lazy_weights_match_deskewed_point_cloud_size);
    RUN(end_to_end);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
