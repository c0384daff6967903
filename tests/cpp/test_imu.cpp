// C++ tests of IMU preintegration and the IMU deskew, included through the reference's paths only: the reference's IMUPreintegration
// cases (cpp/tests/test_imu_preintegration.cpp, restated with their tolerances), its IMUDeskewTest cases
// (cpp/tests/test_imu_deskew.cpp, restated, 5 mm / 5e-3), the in-place call that pins the documented deviation, and the mirrored
// metadata. Built and run by tests/test_gpu_imu_deskew.py on a GPU box; exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

#include "sycl_points/algorithms/deskew/imu_deskew.hpp"
#include "sycl_points/algorithms/deskew/relative_pose_deskew.hpp"
#include "sycl_points/algorithms/imu/imu_preintegration.hpp"

using namespace sycl_points;
namespace imu = sycl_points::imu;
namespace dsk = sycl_points::algorithms::deskew;
using V3 = Eigen::Vector3f;
using M3 = Eigen::Matrix3f;
using M15 = Eigen::Matrix<float, 15, 15>;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); } while (0)

static sycl_utils::DeviceQueue* Q = nullptr;
static constexpr float kEps = 1e-4f, kEpsTight = 1e-5f, kEpsDeskew = 5e-3f;
static constexpr float kPi = 3.14159265358979323846f;

// Eigen's isApprox / isZero on plain arrays
template <class A, class B>
static bool approx(const A& a, const B& b, float prec) {
    double d = 0, na = 0, nb = 0;
    for (int k = 0; k < A::rows() * A::cols(); ++k) {
        d += double(a.data()[k] - b.data()[k]) * double(a.data()[k] - b.data()[k]);
        na += double(a.data()[k]) * a.data()[k];
        nb += double(b.data()[k]) * b.data()[k];
    }
    return std::sqrt(d) <= prec * std::sqrt(std::min(na, nb));
}
template <class A>
static bool is_zero(const A& a, float prec) {
    for (int k = 0; k < A::rows() * A::cols(); ++k)
        if (!(std::fabs(a.data()[k]) <= prec)) return false;
    return true;
}
static M3 rot_z(float a) {
    M3 R = M3::Identity();
    R(0, 0) = std::cos(a); R(0, 1) = -std::sin(a); R(1, 0) = std::sin(a); R(1, 1) = std::cos(a);
    return R;
}
static std::vector<imu::IMUMeasurement> make_constant_imu(double t0, double T, int n_steps, const V3& gyro, const V3& accel) {
    std::vector<imu::IMUMeasurement> meas;
    const double dt = T / n_steps;
    for (int i = 0; i <= n_steps; ++i) {
        imu::IMUMeasurement m;
        m.timestamp = t0 + i * dt;
        m.gyro = gyro;
        m.accel = accel;
        meas.push_back(m);
    }
    return meas;
}
static imu::IMUPreintegrationParams noisy() {
    imu::IMUPreintegrationParams p;
    p.gyro_noise_density = 1e-3f;
    p.accel_noise_density = 1e-2f;
    p.gyro_bias_rw_density = 1e-5f;
    p.accel_bias_rw_density = 1e-4f;
    return p;
}

// ------------------------------------------------------------------------------------------------ IMUPreintegration
static void initial_reset_single() {  // InitialStateIsIdentity, ResetClearsState, SingleMeasurementNoIntegration
    imu::IMUPreintegration integ;
    CHECK(!integ.has_measurements());
    CHECK(integ.get_dt_total() == 0.0);
    CHECK(approx(integ.get_raw().Delta_R, M3::Identity(), kEpsTight));
    CHECK(is_zero(integ.get_raw().Delta_v, kEpsTight) && is_zero(integ.get_raw().Delta_p, kEpsTight));
    integ.integrate_batch(make_constant_imu(0.0, 1.0, 100, V3(0.1f, 0.0f, 0.0f), V3(0.0f, 0.0f, 9.81f)));
    CHECK(integ.has_measurements());
    integ.reset();
    CHECK(!integ.has_measurements());
    CHECK(integ.get_dt_total() == 0.0);
    CHECK(approx(integ.get_raw().Delta_R, M3::Identity(), kEpsTight));
    CHECK(is_zero(integ.get_raw().Delta_v, kEpsTight) && is_zero(integ.get_raw().Delta_p, kEpsTight));
    imu::IMUMeasurement m;
    m.timestamp = 1.0;
    m.gyro = V3(0.1f, 0.2f, 0.3f);
    m.accel = V3(0.0f, 0.0f, 9.81f);
    integ.integrate(m);
    CHECK(integ.has_measurements() && integ.get_dt_total() == 0.0);
    CHECK(approx(integ.get_raw().Delta_R, M3::Identity(), kEpsTight));
}
static void motions() {  // ZeroMotionIdentityResult, ConstantRotationZ, ConstantAccelerationX, DeltaRRemainsValidRotation, Midpoint...
    {
        imu::IMUPreintegration integ;
        integ.integrate_batch(make_constant_imu(0.0, 1.0, 200, V3::Zero(), V3::Zero()));
        const auto& r = integ.get_raw();
        CHECK(approx(r.Delta_R, M3::Identity(), kEps) && is_zero(r.Delta_v, kEps) && is_zero(r.Delta_p, kEps));
        CHECK(std::fabs(r.dt_total - 1.0) <= 1e-9);
    }
    {
        const float omega_z = kPi / 4.0f;
        imu::IMUPreintegration integ;
        integ.integrate_batch(make_constant_imu(0.0, 2.0, 400, V3(0.0f, 0.0f, omega_z), V3::Zero()));
        CHECK(approx(integ.get_raw().Delta_R, rot_z(omega_z * 2.0f), kEps));
    }
    {
        imu::IMUPreintegration integ;
        integ.integrate_batch(make_constant_imu(0.0, 1.5, 300, V3::Zero(), V3(2.0f, 0.0f, 0.0f)));
        const auto& r = integ.get_raw();
        CHECK(std::fabs(r.Delta_p.x() - 0.5f * 2.0f * float(1.5 * 1.5)) <= kEps);
        CHECK(std::fabs(r.Delta_p.y()) <= kEps && std::fabs(r.Delta_p.z()) <= kEps);
        CHECK(std::fabs(r.Delta_v.x() - 2.0f * 1.5f) <= kEps);
    }
    {
        imu::IMUPreintegration integ;
        integ.integrate_batch(make_constant_imu(0.0, 5.0, 500, V3(0.3f, -0.2f, 0.5f), V3(0.1f, 0.2f, 9.5f)));
        const M3 R = integ.get_raw().Delta_R;
        CHECK(approx(R.transpose() * R, M3::Identity(), 1e-4f));
    }
    {
        imu::IMUPreintegration integ;
        integ.integrate_batch(make_constant_imu(0.0, 2.0, 20, V3(0.0f, 0.0f, 1.5f), V3::Zero()));
        CHECK((integ.get_raw().Delta_R - rot_z(1.5f * 2.0f)).norm() < 0.01f);
    }
}
static void batch_and_bias() {  // BatchAndIncrementalAreEqual, BiasCorrection_SmallChange, GetCorrectedSameBiasEqualsRaw
    const auto meas = make_constant_imu(0.0, 1.0, 100, V3(0.05f, -0.03f, 0.08f), V3(0.3f, -0.1f, 9.5f));
    imu::IMUPreintegration inc, batch;
    for (const auto& m : meas) inc.integrate(m);
    batch.integrate_batch(meas);
    CHECK(approx(inc.get_raw().Delta_R, batch.get_raw().Delta_R, kEpsTight) && approx(inc.get_raw().Delta_p, batch.get_raw().Delta_p, kEpsTight));
    CHECK(inc.get_raw().dt_total == batch.get_raw().dt_total);
    imu::IMUBias b0, b1;
    b0.gyro_bias = V3(0.005f, -0.003f, 0.002f);
    b0.accel_bias = V3(0.01f, 0.005f, -0.008f);
    b1.gyro_bias = b0.gyro_bias + V3(0.001f, -0.001f, 0.001f);
    b1.accel_bias = b0.accel_bias + V3(0.002f, 0.001f, -0.001f);
    const auto m2 = make_constant_imu(0.0, 0.5, 100, V3(0.1f, -0.05f, 0.08f), V3(0.2f, 0.1f, 9.7f));
    imu::IMUPreintegration ref, foc;
    ref.reset(b1);
    ref.integrate_batch(m2);
    foc.reset(b0);
    foc.integrate_batch(m2);
    const auto rc = foc.get_corrected(b1);
    CHECK(approx(rc.Delta_R, ref.get_raw().Delta_R, 5e-3f) && approx(rc.Delta_v, ref.get_raw().Delta_v, 5e-3f));
    CHECK(approx(rc.Delta_p, ref.get_raw().Delta_p, 5e-3f));
    const auto same = foc.get_corrected(b0);
    CHECK(approx(same.Delta_R, foc.get_raw().Delta_R, kEpsTight) && approx(same.Delta_v, foc.get_raw().Delta_v, kEpsTight));
    CHECK(approx(same.Delta_p, foc.get_raw().Delta_p, kEpsTight));
}
static void predictions() {  // PredictRelativeTransformZeroMotion, PredictTransform_FreeFall, PredictTransform_InitialVelocity
    {
        imu::IMUPreintegration integ;
        integ.integrate_batch(make_constant_imu(0.0, 0.5, 50, V3::Zero(), -integ.get_params().gravity));
        CHECK(approx(integ.predict_relative_transform(M3::Identity(), V3::Zero(), imu::IMUBias{}), TransformMatrix::Identity(), kEps));
    }
    imu::IMUPreintegrationParams params;
    params.gravity = V3(0.0f, 0.0f, -9.81f);
    {
        imu::IMUPreintegration integ(params);
        integ.integrate_batch(make_constant_imu(0.0, 1.0, 200, V3::Zero(), V3::Zero()));
        const TransformMatrix T = integ.predict_transform(TransformMatrix::Identity(), V3::Zero(), imu::IMUBias{});
        CHECK(std::fabs(T(0, 3)) <= kEps && std::fabs(T(1, 3)) <= kEps && std::fabs(T(2, 3) - 0.5f * -9.81f) <= kEps);
    }
    {
        imu::IMUPreintegration integ(params);
        integ.integrate_batch(make_constant_imu(0.0, 2.0, 400, V3::Zero(), V3::Zero()));
        TransformMatrix Ti = TransformMatrix::Identity();
        Ti(0, 3) = 1.0f; Ti(1, 3) = 2.0f; Ti(2, 3) = 3.0f;
        const TransformMatrix T = integ.predict_transform(Ti, V3(1.0f, -0.5f, 0.0f), imu::IMUBias{});
        CHECK(std::fabs(T(0, 3) - 3.0f) <= kEps && std::fabs(T(1, 3) - 1.0f) <= kEps);
        CHECK(std::fabs(T(2, 3) - (3.0f + 0.5f * -9.81f * 4.0f)) <= kEps);
    }
}
static void covariances() {  // the covariance TESTs (14-20, 23, 24)
    {
        imu::IMUPreintegration integ;
        integ.integrate_batch(make_constant_imu(0.0, 1.0, 100, V3(0.1f, 0.0f, 0.0f), V3(0.0f, 0.0f, 9.81f)));
        CHECK(is_zero(integ.get_raw().covariance, kEpsTight));
    }
    {
        imu::IMUPreintegration integ(noisy());
        integ.integrate_batch(make_constant_imu(0.0, 1.0, 100, V3(0.1f, -0.05f, 0.08f), V3(0.2f, 0.1f, 9.7f)));
        const M15 cov = integ.get_raw().covariance;
        CHECK(cov(3, 3) > 0 && cov(6, 6) > 0 && cov(0, 0) > 0 && cov(9, 9) > 0 && cov(12, 12) > 0);
        CHECK(approx(cov, cov.transpose(), 1e-5f));
    }
    {
        M15 P0 = M15::Zero();
        for (int k = 0; k < 3; ++k) P0(6 + k, 6 + k) = 1e-4f;
        imu::IMUPreintegration integ;
        integ.reset(imu::IMUBias{}, P0);
        imu::IMUMeasurement m0;
        integ.integrate(m0);
        CHECK(approx(integ.get_raw().covariance, P0, kEpsTight));  // no step yet
        integ.reset(imu::IMUBias{}, P0);
        integ.integrate_batch(make_constant_imu(0.0, 1.0, 100, V3::Zero(), V3::Zero()));
        const M15 cov = integ.get_raw().covariance;
        CHECK(std::fabs(cov(6, 6) - P0(6, 6)) <= 1e-6f && cov(0, 0) > 0 && cov(1, 1) > 0 && cov(2, 2) > 0);
    }
    {  // CovarianceUsesWorldFrameAtReset
        const float dt = 0.1f;
        const M3 Rwb = rot_z(kPi / 2.0f);
        const V3 accel(1.0f, 2.0f, 9.0f);
        M15 P0 = M15::Zero();
        M3 P_rot = M3::Zero();
        P_rot(0, 0) = 1e-4f; P_rot(1, 1) = 2e-4f; P_rot(2, 2) = 3e-4f;
        for (int i = 0; i < 3; ++i) P0(3 + i, 3 + i) = P_rot(i, i);
        imu::IMUPreintegration integ;
        integ.reset(imu::IMUBias{}, P0, Rwb);
        integ.integrate_batch(make_constant_imu(0.0, dt, 1, V3::Zero(), accel));
        M3 S = M3::Zero();
        S(0, 1) = -accel[2]; S(0, 2) = accel[1]; S(1, 0) = accel[2]; S(1, 2) = -accel[0]; S(2, 0) = -accel[1]; S(2, 1) = accel[0];
        const M3 A = (-Rwb * S) * dt;
        const M3 expected = A * P_rot * A.transpose();
        M3 actual;
        const M15 cov = integ.get_raw().covariance;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) actual(i, j) = cov(6 + i, 6 + j);
        CHECK(approx(actual, expected, 1e-6f));
    }
    {  // GyroNoiseCouplesIntoPositionAndVelocity
        imu::IMUPreintegrationParams p;
        p.gyro_noise_density = 1e-2f;
        imu::IMUPreintegration integ(p);
        integ.integrate_batch(make_constant_imu(0.0, 0.1, 1, V3(0.0f, 0.0f, 1.0f), V3(4.0f, 1.0f, 8.0f)));
        const M15 cov = integ.get_raw().covariance;
        CHECK(cov(0, 0) + cov(1, 1) + cov(2, 2) > 0 && cov(6, 6) + cov(7, 7) + cov(8, 8) > 0);
        float cross = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) cross += cov(6 + i, 3 + j) * cov(6 + i, 3 + j);
        CHECK(cross > 0);
    }
}
static void jacobians_and_window() {  // MidpointGyroBiasJacobiansMatchFiniteDifference, MeasurementWindowInterpolatesBoundaries
    const float eps = 1e-2f;
    const auto meas = make_constant_imu(0.0, 0.2, 1, V3(0.2f, -0.1f, 1.0f), V3(4.0f, 1.0f, 8.0f));
    imu::IMUPreintegration nominal, plus, minus;
    nominal.integrate_batch(meas);
    imu::IMUBias bp, bm;
    bp.gyro_bias.z() = eps;
    bm.gyro_bias.z() = -eps;
    plus.reset(bp);
    plus.integrate_batch(meas);
    minus.reset(bm);
    minus.integrate_batch(meas);
    const V3 num_v = (plus.get_raw().Delta_v - minus.get_raw().Delta_v) / (2.0f * eps);
    const V3 num_p = (plus.get_raw().Delta_p - minus.get_raw().Delta_p) / (2.0f * eps);
    const M3 Jv = nominal.get_raw().J.J_v_bg, Jp = nominal.get_raw().J.J_p_bg;
    CHECK(approx(V3(Jv(0, 2), Jv(1, 2), Jv(2, 2)), num_v, 5e-4f));
    CHECK(approx(V3(Jp(0, 2), Jp(1, 2), Jp(2, 2)), num_p, 5e-4f));
    std::vector<imu::IMUMeasurement> ms(3), window;
    for (size_t i = 0; i < 3; ++i) {
        ms[i].timestamp = double(i);
        ms[i].gyro = V3(float(i), float(i), float(i));
        ms[i].accel = V3(10.0f * i, 10.0f * i, 10.0f * i);
    }
    imu::build_measurement_window(ms, 0.25, 1.75, window);
    CHECK(window.size() == 3u);
    if (window.size() == 3u) {
        CHECK(window[0].timestamp == 0.25 && window[1].timestamp == 1.0 && window[2].timestamp == 1.75);
        CHECK(approx(window[0].gyro, V3(0.25f, 0.25f, 0.25f), 1e-5f) && approx(window[2].accel, V3(17.5f, 17.5f, 17.5f), 1e-5f));
    }
}

// ------------------------------------------------------------------------------------------------ IMUDeskewTest
static std::deque<imu::IMUMeasurement> make_imu_buffer(double t0, double T, int n_steps, const V3& gyro, const V3& force) {
    const auto v = make_constant_imu(t0, T, n_steps, gyro, force);
    return std::deque<imu::IMUMeasurement>(v.begin(), v.end());
}
static imu::IMUPreintegrationParams no_gravity() {
    imu::IMUPreintegrationParams p;
    p.gravity = V3::Zero();
    return p;
}
static V3 unrotate_z(double angle, const V3& w) {  // R_z(angle)^T w
    const double c = std::cos(angle), s = std::sin(angle);
    return V3(float(c * w[0] + s * w[1]), float(-s * w[0] + c * w[1]), w[2]);
}
static float dist3(const PointType& p, const V3& w) {
    return std::sqrt((p[0] - w[0]) * (p[0] - w[0]) + (p[1] - w[1]) * (p[1] - w[1]) + (p[2] - w[2]) * (p[2] - w[2]));
}
static void pure_rotation_and_gyro_only_twin() {
    PointCloudShared cloud(*Q);
    const double start = 1.0, duration = 0.1;
    cloud.start_time_ms = start * 1e3;
    cloud.end_time_ms = (start + duration) * 1e3;
    const float omega_z = kPi / 2.0f;
    const std::vector<V3> world = {V3(1, 0, 0), V3(0, 1, 0), V3(1, 1, 0.5f), V3(-1, 0.5f, 0), V3(0.5f, -0.5f, 1)};
    const std::vector<float> off = {0.0f, 25.0f, 50.0f, 75.0f, 100.0f};
    for (size_t i = 0; i < world.size(); ++i) {
        const V3 p = unrotate_z(double(omega_z) * off[i] * 1e-3, world[i]);
        cloud.points->push_back(PointType(p[0], p[1], p[2], 1.0f));
        cloud.timestamp_offsets->push_back(off[i]);
    }
    const auto buf = make_imu_buffer(start - 0.02, duration + 0.04, 24, V3(0, 0, omega_z), V3::Zero());
    for (bool gyro_only : {false, true}) {
        PointCloudShared out(*Q);
        dsk::IMUDeskewStatus status;
        const bool ok = dsk::deskew_point_cloud_imu(cloud, out, buf, start, Eigen::Isometry3f::Identity(), imu::IMUBias(), no_gravity(),
                                                    M3::Identity(), V3::Zero(), &status, gyro_only);
        CHECK(ok && status == dsk::IMUDeskewStatus::success && out.size() == world.size());
        if (!ok) continue;
        for (size_t i = 0; i < world.size(); ++i) CHECK(dist3((*out.points)[i], world[i]) <= kEpsDeskew);
        CHECK(out.start_time_ms == cloud.start_time_ms && out.end_time_ms == cloud.end_time_ms);  // the metadata is the input's
        CHECK(out.timestamp_offsets->size() == off.size() && (*out.timestamp_offsets)[3] == off[3]);
        CHECK(!out.has_normal() && !out.has_cov());
    }
}
static void pure_translation() {
    PointCloudShared cloud(*Q);
    const double start = 2.0;
    cloud.start_time_ms = start * 1e3;
    cloud.end_time_ms = (start + 0.1) * 1e3;
    const std::vector<V3> world = {V3(2, 0, 0), V3(0, 2, 0), V3(1, 1, 1)};
    const std::vector<float> off = {0.0f, 50.0f, 100.0f};
    for (size_t i = 0; i < world.size(); ++i) {
        const float t = off[i] * 1e-3f;
        cloud.points->push_back(PointType(world[i][0] - 0.5f * t * t, world[i][1], world[i][2], 1.0f));
        cloud.timestamp_offsets->push_back(off[i]);
    }
    const auto buf = make_imu_buffer(start - 0.02, 0.14, 24, V3::Zero(), V3(1.0f, 0, 0));
    PointCloudShared out(*Q);
    dsk::IMUDeskewStatus status;
    CHECK(dsk::deskew_point_cloud_imu(cloud, out, buf, start, Eigen::Isometry3f::Identity(), imu::IMUBias(), no_gravity(), M3::Identity(),
                                      V3::Zero(), &status));
    for (size_t i = 0; i < world.size() && i < out.size(); ++i) CHECK(dist3((*out.points)[i], world[i]) <= kEpsDeskew);
}
static void gyro_only_ignores_acceleration_and_velocity() {
    PointCloudShared cloud(*Q);
    const double start = 3.0;
    cloud.start_time_ms = start * 1e3;
    cloud.end_time_ms = (start + 0.1) * 1e3;
    const std::vector<V3> in = {V3(1, 2, 3), V3(-2, 0.5f, 1), V3(0.25f, -0.75f, 4)};
    const std::vector<float> off = {0.0f, 50.0f, 100.0f};
    for (size_t i = 0; i < in.size(); ++i) {
        cloud.points->push_back(PointType(in[i][0], in[i][1], in[i][2], 1.0f));
        cloud.timestamp_offsets->push_back(off[i]);
    }
    const auto buf = make_imu_buffer(start - 0.02, 0.14, 24, V3::Zero(), V3(3.0f, -2.0f, 11.0f));
    PointCloudShared out(*Q);
    dsk::IMUDeskewStatus status;
    CHECK(dsk::deskew_point_cloud_imu(cloud, out, buf, start, Eigen::Isometry3f::Identity(), imu::IMUBias(), imu::IMUPreintegrationParams(),
                                      M3::Identity(), V3(5.0f, -4.0f, 2.0f), &status, true));
    for (size_t i = 0; i < in.size() && i < out.size(); ++i) CHECK(dist3((*out.points)[i], in[i]) <= kEpsDeskew);
}
static void status_cases() {  // InsufficientIMUData, NoTimestamps, ZeroScanDuration, PartialIMUCoverage, and an empty cloud
    auto one = [](double s_ms, double e_ms, bool stamps) {
        PointCloudShared c(*Q);
        c.start_time_ms = s_ms;
        c.end_time_ms = e_ms;
        c.points->push_back(PointType(1, 0, 0, 1));
        if (stamps) c.timestamp_offsets->push_back(0.0f);
        return c;
    };
    auto run = [](const PointCloudShared& c, const std::deque<imu::IMUMeasurement>& buf, dsk::IMUDeskewStatus& st) {
        PointCloudShared out(*Q);
        return dsk::deskew_point_cloud_imu(c, out, buf, 1.0, Eigen::Isometry3f::Identity(), imu::IMUBias(), imu::IMUPreintegrationParams(),
                                           M3::Identity(), V3::Zero(), &st);
    };
    const auto full = make_imu_buffer(0.98, 0.14, 20, V3::Zero(), V3(0, 0, 9.81f));
    dsk::IMUDeskewStatus st = dsk::IMUDeskewStatus::success;
    CHECK(!run(one(1000.0, 1100.0, true), {}, st) && st == dsk::IMUDeskewStatus::insufficient_imu_coverage);
    CHECK(!run(one(1000.0, 1100.0, false), full, st) && st == dsk::IMUDeskewStatus::no_timestamps);
    CHECK(!run(one(1000.0, 1000.0, true), full, st) && st == dsk::IMUDeskewStatus::invalid_scan_duration);
    CHECK(!run(one(1000.0, 1100.0, true), make_imu_buffer(0.98, 0.06, 10, V3::Zero(), V3(0, 0, 9.81f)), st) &&
          st == dsk::IMUDeskewStatus::insufficient_imu_coverage);
    PointCloudShared empty(*Q);
    CHECK(!run(empty, full, st) && st == dsk::IMUDeskewStatus::empty_cloud);
    CHECK(run(one(1000.0, 1100.0, true), full, st) && st == dsk::IMUDeskewStatus::success);
}
// NormalsAndCovariancesRotated, then the same call in place: the rotated attributes, not the reference's zeros
static void normals_and_covariances_rotated_also_in_place() {
    PointCloudShared cloud(*Q);
    cloud.start_time_ms = 0.0;
    cloud.end_time_ms = 100.0;
    const float omega_z = kPi / 2.0f;
    const V3 wp(1, 1, 0), wn(0, 0, 1);
    const float wc[3] = {0.01f, 0.02f, 0.03f};
    const std::vector<float> off = {0.0f, 50.0f, 100.0f};
    for (float o : off) {
        const double a = double(omega_z) * o * 1e-3, c = std::cos(a), s = std::sin(a);
        const double Rt[3][3] = {{c, s, 0}, {-s, c, 0}, {0, 0, 1}};  // pose^T
        const V3 p = unrotate_z(a, wp);
        cloud.points->push_back(PointType(p[0], p[1], p[2], 1.0f));
        cloud.timestamp_offsets->push_back(o);
        cloud.normals->push_back(Normal(0, 0, 1, 0));
        Covariance C = Covariance::Zero();
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) C(i, j) = float(Rt[i][0] * wc[0] * Rt[j][0] + Rt[i][1] * wc[1] * Rt[j][1] + Rt[i][2] * wc[2] * Rt[j][2]);
        cloud.covs->push_back(C);
    }
    const auto buf = make_imu_buffer(-0.02, 0.14, 24, V3(0, 0, omega_z), V3::Zero());
    auto check = [&](const PointCloudShared& out) {
        for (size_t i = 0; i < off.size(); ++i) {
            CHECK(dist3((*out.points)[i], wp) <= kEpsDeskew);
            CHECK(dist3((*out.normals)[i], wn) <= kEpsDeskew && (*out.normals)[i][3] == 0.0f);
            double d = 0;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) d += std::pow(double((*out.covs)[i](r, c)) - (r == c ? wc[r] : 0.0), 2);
            CHECK(std::sqrt(d) <= kEpsDeskew);
            CHECK((*out.covs)[i](3, 3) == 0.0f && (*out.covs)[i](0, 3) == 0.0f);
        }
    };
    PointCloudShared out(*Q);
    CHECK(dsk::deskew_point_cloud_imu(cloud, out, buf, 0.0, Eigen::Isometry3f::Identity(), imu::IMUBias(), no_gravity(), M3::Identity(),
                                      V3::Zero()));
    check(out);
    dsk::IMUDeskewStatus st;
    CHECK(dsk::deskew_point_cloud_imu(cloud, cloud, buf, 0.0, Eigen::Isometry3f::Identity(), imu::IMUBias(), no_gravity(), M3::Identity(),
                                      V3::Zero(), &st));
    check(cloud);
    for (size_t i = 0; i < off.size(); ++i) {  // in place equals out of place bit for bit
        CHECK(std::memcmp((*cloud.points)[i].data(), (*out.points)[i].data(), 16) == 0);
        CHECK(std::memcmp((*cloud.covs)[i].data(), (*out.covs)[i].data(), 64) == 0);
        CHECK(std::memcmp((*cloud.normals)[i].data(), (*out.normals)[i].data(), 16) == 0);
    }
}
// The output side of the call, which the constant-velocity deskew shares: out of place, an output cloud that held other rows and
// attributes ends up with the input's rgb, stamps and times and without the attributes the input does not have; in place leaves
// them alone
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
    const auto buf = make_imu_buffer(1.0 - 0.02, 0.14, 24, V3(0, 0, kPi / 2.0f), V3::Zero());
    CHECK(dsk::deskew_point_cloud_imu(cloud, out, buf, 1.0, Eigen::Isometry3f::Identity(), imu::IMUBias(), no_gravity(), M3::Identity(),
                                      V3::Zero()));
    CHECK(untouched(out));
    CHECK(dsk::deskew_point_cloud_imu(cloud, cloud, buf, 1.0, Eigen::Isometry3f::Identity(), imu::IMUBias(), no_gravity(), M3::Identity(),
                                      V3::Zero()));
    CHECK(untouched(cloud));
    CHECK(std::memcmp(cloud.points->host().data(), out.points->host().data(), 8 * sizeof(PointType)) == 0);
}
static void matches_constant_velocity_approximately() {
    const float omega_z = kPi / 4.0f;
    TransformMatrix end = TransformMatrix::Identity();
    const M3 Re = rot_z(omega_z * 0.1f);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) end(i, j) = Re(i, j);
    const V3 wp(1.0f, 0.5f, 0.0f);
    PointCloudShared cloud(*Q);
    cloud.start_time_ms = 0.0;
    cloud.end_time_ms = 100.0;
    for (float o : {0.0f, 50.0f, 100.0f}) {
        const V3 p = unrotate_z(double(omega_z) * o * 1e-3, wp);
        cloud.points->push_back(PointType(p[0], p[1], p[2], 1.0f));
        cloud.timestamp_offsets->push_back(o);
    }
    const auto buf = make_imu_buffer(-0.02, 0.14, 24, V3(0, 0, omega_z), V3::Zero());
    PointCloudShared d_imu(*Q), d_cv(*Q);
    CHECK(dsk::deskew_point_cloud_imu(cloud, d_imu, buf, 0.0, Eigen::Isometry3f::Identity(), imu::IMUBias(), no_gravity(), M3::Identity(),
                                      V3::Zero()));
    CHECK(dsk::deskew_point_cloud_constant_velocity(cloud, d_cv, Eigen::Isometry3f::Identity(), Eigen::Isometry3f(end)));
    for (size_t i = 0; i < 3 && i < d_imu.size() && i < d_cv.size(); ++i) {
        CHECK(dist3((*d_imu.points)[i], wp) <= kEpsDeskew);
        CHECK(dist3((*d_cv.points)[i], wp) <= kEpsDeskew);
    }
}

int main() {
    sycl_utils::DeviceQueue queue;
    Q = &queue;
    RUN(initial_reset_single);
    RUN(motions);
    RUN(batch_and_bias);
    RUN(predictions);
    RUN(covariances);
    RUN(jacobians_and_window);
    RUN(pure_rotation_and_gyro_only_twin);
    RUN(pure_translation);
    RUN(gyro_only_ignores_acceleration_and_velocity);
    RUN(status_cases);
    RUN(normals_and_covariances_rotated_also_in_place);
    RUN(output_takes_the_attributes_the_deskew_does_not_touch);
    RUN(matches_constant_velocity_approximately);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
