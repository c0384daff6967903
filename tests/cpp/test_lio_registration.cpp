// C++ tests of lio::LIORegistration and its building blocks, included through the reference's six paths only, so reference-style
// code compiles against the facade. Built and run by tests/test_gpu_lio.py on a GPU box: test_lio_registration <golden dir>;
// exit code 0 = all checks passed.
//   1. the two known answers of the reference's test_lio_registration.cpp and three of its test_imu_factor.cpp (tolerances 1e-5 /
//      1e-6), through the facade types
//   2. align() is the stepper chain (LM / GICP / KDTree, a 600-of-900-point synthetic pair): against sp_lio_stepper_* driven by
//      hand from a fresh Registration - bit for bit when two hand runs agree bit for bit, else within four times their difference
//   3. on the golden pair (box filter, voxel grid 0.25, k = 10 covariances) from the ground truth moved by (0.01, -0.005, 0.02 rad;
//      0.05, -0.04, 0.03 m): a loose prior ends within twice the pose error of Registration::align; a tight prior
//      (h >= 100 |H_icp|_F) keeps the prediction within 2 |b_icp| / h
// Every figure is printed before it is checked.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "sycl_points/algorithms/imu/imu_factor.hpp"
#include "sycl_points/algorithms/lio/lio_linearized_result.hpp"
#include "sycl_points/algorithms/lio/lio_registration.hpp"
#include "sycl_points/algorithms/lio/lio_registration_params.hpp"
#include "sycl_points/algorithms/lio/lio_registration_result.hpp"
#include "sycl_points/algorithms/registration/dogleg_step.hpp"

#include "sycl_points/algorithms/common/transform.hpp"
#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/filter/voxel_downsampling.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"

using namespace sycl_points;
namespace alg = sycl_points::algorithms;
namespace lio = sycl_points::algorithms::lio;
namespace reg = sycl_points::algorithms::registration;
using M3 = Eigen::Matrix3f;
using M4 = Eigen::Matrix4f;
using M15 = Eigen::Matrix<float, 15, 15>;
using V15 = Eigen::Matrix<float, 15, 1>;

static int g_failed = 0, g_checks = 0;
#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) { ++g_failed; std::printf("  CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)
#define RUN(fn) do { std::printf("[ RUN  ] %s\n", #fn); std::fflush(stdout); const int before = g_failed; fn(); std::printf("[ %s ] %s\n", g_failed == before ? " OK " : "FAIL", #fn); std::fflush(stdout); } while (0)

static sycl_utils::DeviceQueue* Q = nullptr;
static std::string g_dir;

static M15 diag15(float v) {
    M15 m = M15::Zero();
    for (int i = 0; i < 15; ++i) m(i, i) = v;
    return m;
}
static M3 rot_z(float a) {
    M3 R = M3::Identity();
    R(0, 0) = std::cos(a); R(0, 1) = -std::sin(a); R(1, 0) = std::sin(a); R(1, 1) = std::cos(a);
    return R;
}
static bool near(float a, float b, float eps) { return std::fabs(a - b) <= eps; }

// ------------------------------------------------------------------------------------------------ 1. known answers
static void known_answers_lio() {
    {  // DirectionalIcpWeightingAttenuatesWeakDirections
        lio::LIOLinearizedResult f;
        f.inlier = 100;
        f.H(imu::State::kIdxPos, imu::State::kIdxPos) = 1.0f;
        f.H(imu::State::kIdxPos + 1, imu::State::kIdxPos + 1) = 20.0f;
        f.H(imu::State::kIdxRot, imu::State::kIdxRot) = 1.0f;
        f.b(imu::State::kIdxPos) = 10.0f;
        f.b(imu::State::kIdxPos + 1) = 20.0f;
        f.b(imu::State::kIdxRot) = 10.0f;
        lio::DirectionalIcpWeightingParams p;
        p.trans_min_eigenvalue_per_inlier = 0.05f;
        p.rot_min_eigenvalue_per_inlier = 0.05f;
        p.trans_weak_direction_scale = 0.1f;
        p.rot_weak_direction_scale = 0.25f;
        lio::apply_directional_icp_weighting(f, p);
        std::printf("  weak directions: H %.7g %.7g %.7g, b %.7g %.7g %.7g\n", f.H(0, 0), f.H(1, 1), f.H(3, 3), f.b(0), f.b(1), f.b(3));
        CHECK(near(f.H(0, 0), 0.2f, 1e-5f) && near(f.b(0), 2.0f, 1e-5f));
        CHECK(near(f.H(1, 1), 20.0f, 1e-5f) && near(f.b(1), 20.0f, 1e-5f));
        CHECK(near(f.H(3, 3), 0.25f, 1e-5f) && near(f.b(3), 2.5f, 1e-5f));
    }
    {  // DirectionalIcpWeightingPreservesCoupledFactorStructure
        lio::LIOLinearizedResult f;
        f.inlier = 100;
        f.H(0, 0) = 1.0f; f.H(3, 3) = 1.0f; f.H(0, 3) = 0.5f; f.H(3, 0) = 0.5f;
        lio::DirectionalIcpWeightingParams p;
        p.trans_min_eigenvalue_per_inlier = 0.1f;
        p.rot_min_eigenvalue_per_inlier = 0.1f;
        p.trans_weak_direction_scale = 0.1f;
        p.rot_weak_direction_scale = 0.4f;
        lio::apply_directional_icp_weighting(f, p);
        std::printf("  coupled: H %.7g %.7g %.7g %.7g\n", f.H(0, 0), f.H(3, 3), f.H(0, 3), f.H(3, 0));
        CHECK(near(f.H(0, 0), 0.1f, 1e-5f) && near(f.H(3, 3), 0.4f, 1e-5f) && near(f.H(0, 3), 0.1f, 1e-5f) && near(f.H(3, 0), 0.1f, 1e-5f));
        // the 2x2 system [[0.1, 0.1], [0.1, 0.4]] is positive definite; nothing else is non-zero
        CHECK(f.H(0, 0) * f.H(3, 3) - f.H(0, 3) * f.H(3, 0) > 0.0f);
    }
}

static void known_answers_imu() {
    {  // HessianIsInverseOfCovariance
        imu::State a, b;
        M15 H;
        V15 g;
        CHECK(imu::compute_imu_hessian_gradient(a, b, diag15(0.04f), H, g));
        float worst = 0.0f;
        for (int i = 0; i < 15; ++i)
            for (int j = 0; j < 15; ++j) worst = std::max(worst, std::fabs(H(i, j) * 0.04f - (i == j ? 1.0f : 0.0f)));
        std::printf("  |H P - I| = %.3g\n", worst);
        CHECK(worst <= 1e-6f);
    }
    {  // RotationResidualSO3Log
        imu::State a, b;
        const float angle = 3.14159265358979323846f / 6.0f;
        b.rotation = rot_z(angle);
        M15 H;
        V15 g;
        CHECK(imu::compute_imu_hessian_gradient(a, b, diag15(1.0f), H, g));
        std::printf("  rotation residual %.7g %.7g %.7g (angle %.7g)\n", g(3), g(4), g(5), angle);
        CHECK(near(g(3), 0.0f, 1e-5f) && near(g(4), 0.0f, 1e-5f) && near(g(5), angle, 1e-5f));
        for (int i = 0; i < 15; ++i)
            if (i < 3 || i >= 6) CHECK(std::fabs(g(i)) <= 1e-6f);
        const V15 r = imu::compute_manifold_residual(a, b);
        CHECK(near(r(5), angle, 1e-5f));
    }
    {  // IllConditionedCovarianceReturnsZero
        imu::State a, b;
        b.position = Eigen::Vector3f(1.0f, 2.0f, 3.0f);
        M15 H = diag15(7.0f);
        V15 g;
        g(0) = 7.0f;
        CHECK(!imu::compute_imu_hessian_gradient(a, b, M15::Zero(), H, g));
        bool zero = true;
        for (int i = 0; i < 225; ++i) zero = zero && H.data()[i] == 0.0f;
        for (int i = 0; i < 15; ++i) zero = zero && g(i) == 0.0f;
        CHECK(zero);
    }
    static_assert(imu::State::kIdxPos == 0 && imu::State::kIdxRot == 3 && imu::State::kIdxVel == 6 && imu::State::kIdxAccBias == 9 &&
                  imu::State::kIdxGyrBias == 12 && imu::State::kDOF == 15);
    {  // the dog-leg step of both sizes compiles and takes the Gauss-Newton point inside a wide region: H = 2 I, g = 1 -> p = -0.5
        Eigen::Matrix<float, 6, 6> H6 = Eigen::Matrix<float, 6, 6>::Zero();
        Eigen::Vector<float, 6> g6;
        M15 H15 = diag15(2.0f);
        V15 g15;
        for (int i = 0; i < 6; ++i) { H6(i, i) = 2.0f; g6(i) = 1.0f; }
        for (int i = 0; i < 15; ++i) g15(i) = 1.0f;
        const reg::DoglegStep<6> s6 = reg::compute_dogleg_step<6>(H6, g6, 10.0f);
        const reg::DoglegStep<15> s15 = reg::compute_dogleg_step<15>(H15, g15, 10.0f);
        std::printf("  dog-leg: p %.7g / %.7g, norm %.7g / %.7g, predicted %.7g / %.7g\n", s6.p(0), s15.p(14), s6.step_norm, s15.step_norm,
                    s6.predicted_reduction, s15.predicted_reduction);
        CHECK(near(s6.p(0), -0.5f, 1e-6f) && near(s15.p(14), -0.5f, 1e-6f));
        CHECK(near(s6.step_norm, 0.5f * std::sqrt(6.0f), 1e-6f) && near(s15.step_norm, 0.5f * std::sqrt(15.0f), 1e-6f));
        CHECK(near(s6.predicted_reduction, 1.5f, 1e-6f) && near(s15.predicted_reduction, 3.75f, 1e-6f));
    }
}

// ------------------------------------------------------------------------------------------------ helpers
static M4 moved(const M4& T_gt) {  // the ground truth moved by (0.01, -0.005, 0.02 rad; 0.05, -0.04, 0.03 m)
    const float twist[6] = {0.01f, -0.005f, 0.02f, 0.0f, 0.0f, 0.0f};
    M4 D;
    sp_se3_exp_host(twist, D.data());
    D(0, 3) = 0.05f; D(1, 3) = -0.04f; D(2, 3) = 0.03f;
    M4 out;
    sp_rigid_mul_host(T_gt.data(), D.data(), out.data());
    return out;
}
static imu::State predicted(const M4& T) {
    imu::State s;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) s.rotation(i, j) = T(i, j);
        s.position(i) = T(i, 3);
    }
    s.velocity = Eigen::Vector3f(0.3f, -0.2f, 0.1f);
    s.accel_bias = Eigen::Vector3f(0.02f, -0.01f, 0.03f);
    s.gyro_bias = Eigen::Vector3f(0.001f, 0.002f, -0.001f);
    return s;
}
static M4 pose_of(const imu::State& s) {
    M4 T = M4::Identity();
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T(i, j) = s.rotation(i, j);
        T(i, 3) = s.position(i);
    }
    return T;
}
/// translation distance and rotation angle between two poses
static void pose_error(const M4& A, const M4& B, float* trans, float* angle) {
    const float d[3] = {A(0, 3) - B(0, 3), A(1, 3) - B(1, 3), A(2, 3) - B(2, 3)};
    *trans = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    M4 Bi = M4::Identity(), rel;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Bi(i, j) = B(j, i);
    M4 Ar = M4::Identity();
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Ar(i, j) = A(i, j);
    sp_rigid_mul_host(Bi.data(), Ar.data(), rel.data());
    float tw[6];
    sp_se3_log_host(rel.data(), tw);
    *angle = std::sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]);
}
static void with_covariances(PointCloudShared& cloud, size_t k) {
    const auto tree = alg::knn::KDTree::build(*Q, cloud);
    alg::covariance::estimate_async(tree->knn_search(cloud, k), cloud).wait_and_throw();
}

struct HandResult {
    float state[21];
    float posterior[225];
    uint32_t iterations, inlier;
    float error;
};
/// LIORegistration::align written out: sp_lio_stepper_* served by a fresh Registration
static HandResult hand_align(const reg::RegistrationFactorParams& factor, const sp_lio_params& prm, const PointCloudShared& source,
                             const PointCloudShared& target, const alg::knn::KNNBase& knn, const imu::State& pred, const M15& P,
                             const M15& P_prev, bool update_bias) {
    reg::Registration registration(*Q, reg::RegistrationParams(factor));
    const bool plane = factor.reg_type == reg::RegType::POINT_TO_PLANE || factor.reg_type == reg::RegType::GENZ;
    const sp_lio_factor_facts facts{plane ? 1 : 3, factor.robust.type == alg::robust::RobustLossType::NONE ? 1 : 0, factor.robust.default_scale,
                                    factor.rotation_constraint.robust.default_scale};
    const M4 initial_pose = pose_of(pred);
    sp_lio_stepper* h = nullptr;
    throw_on_error(sp_lio_stepper_create(&prm, &facts, imu::detail::PackedState(pred).v, P.data(), P_prev.data(), update_bias ? 1 : 0, &h));
    const std::unique_ptr<sp_lio_stepper, void (*)(sp_lio_stepper*)> guard(h, sp_lio_stepper_destroy);
    sp_lio_request req;
    reg::Registration::ExecutionOptions options;
    for (;;) {
        throw_on_error(sp_lio_stepper_next(h, &req));
        if (req.want == SP_OPT_WANT_DONE) break;
        options.robust_scale = req.robust_scale;
        options.rotation_robust_scale = req.rotation_robust_scale;
        M4 pose;
        std::memcpy(pose.data(), req.T, sizeof(req.T));
        if (req.want == SP_OPT_WANT_LINEARIZE) {
            const sp_linearized lin = lio::detail::to_c(registration.compute_linearized_result(source, target, knn, pose, initial_pose, options));
            throw_on_error(sp_lio_stepper_linearized(h, &lin));
        } else {
            const auto [error, inlier] = registration.compute_error_frozen(source, target, pose, options);
            throw_on_error(sp_lio_stepper_trial(h, error, inlier));
        }
    }
    sp_lio_result res;
    throw_on_error(sp_lio_stepper_result(h, &res));
    HandResult out;
    std::memcpy(out.state, res.state, sizeof(out.state));
    std::memcpy(out.posterior, res.posterior_covariance, sizeof(out.posterior));
    out.iterations = res.iterations;
    out.inlier = res.inlier;
    out.error = res.error;
    return out;
}
static float hand_diff(const HandResult& a, const HandResult& b) {
    float d = 0.0f;
    for (int i = 0; i < 21; ++i) d = std::max(d, std::fabs(a.state[i] - b.state[i]));
    for (int i = 0; i < 225; ++i) d = std::max(d, std::fabs(a.posterior[i] - b.posterior[i]));
    d = std::max(d, std::fabs(a.error - b.error));
    d = std::max(d, std::fabs(float(a.iterations) - float(b.iterations)));
    return std::max(d, std::fabs(float(a.inlier) - float(b.inlier)));
}

// ------------------------------------------------------------------------------------------------ 2. the chain
static void align_is_the_stepper_chain() {
    const size_t n = 900, m = 600;
    std::mt19937 gen(1234);
    const float range = 10.0f * std::cbrt(float(n) * 8.0f / 1e6f);
    std::uniform_real_distribution<float> uni(-range, range);
    PointCloudCPU tc;
    tc.points->resize(n);
    for (size_t i = 0; i < n; ++i) (*tc.points)[i] = PointType(uni(gen), uni(gen), uni(gen), 1.0f);
    const float twist[6] = {0.01f, -0.02f, 0.015f, 0.03f, -0.02f, 0.01f};
    M4 T_gt;
    sp_se3_exp_host(twist, T_gt.data());
    PointCloudShared target(*Q, tc);
    PointCloudShared all = alg::transform::transform_copy(target, Eigen::Isometry3f(T_gt).inverse().matrix());
    std::mt19937 ngen(4321);
    std::normal_distribution<float> noise(0.0f, 0.005f);
    PointCloudCPU sc;
    sc.points->resize(m);
    for (size_t i = 0; i < m; ++i) {
        PointType p = (*all.points)[i];
        p.x() += noise(ngen); p.y() += noise(ngen); p.z() += noise(ngen);
        (*sc.points)[i] = p;
    }
    PointCloudShared source(*Q, sc);
    with_covariances(source, 20);
    with_covariances(target, 20);
    const auto tree = alg::knn::KDTree::build(*Q, target);

    reg::RegistrationFactorParams factor;  // GICP
    lio::LIORegistrationParams params;
    params.total_iterations = 6;
    params.optimization.optimization_method = reg::OptimizationMethod::LEVENBERG_MARQUARDT;
    const imu::State pred = predicted(moved(T_gt));
    M15 P = diag15(2e-3f);
    for (int i = 0; i < 14; ++i) { P(i, i + 1) = 5e-4f; P(i + 1, i) = 5e-4f; }  // couples neighbouring components, stays positive definite
    const M15 P_prev = diag15(0.125f);

    const sp_lio_params prm = lio::detail::to_c(params);
    const HandResult a = hand_align(factor, prm, source, target, *tree, pred, P, P_prev, true);
    const HandResult b = hand_align(factor, prm, source, target, *tree, pred, P, P_prev, true);
    lio::LIORegistration lio_reg(*Q, factor, params);
    CHECK(lio_reg.registration_backend() != nullptr);
    const lio::LIORegistrationResult r = lio_reg.align(source, target, *tree, pred, P, P_prev, true, 0.1f, M4::Identity());
    HandResult got;
    std::memcpy(got.state, imu::detail::PackedState(r.state).v, sizeof(got.state));
    std::memcpy(got.posterior, r.posterior_covariance.data(), sizeof(got.posterior));
    got.iterations = uint32_t(r.registration_result.iterations);
    got.inlier = r.registration_result.inlier;
    got.error = r.registration_result.error;
    const float spread = hand_diff(a, b), diff = hand_diff(got, a);
    float dt, da;
    pose_error(r.registration_result.T.matrix(), T_gt, &dt, &da);
    std::printf("  iterations %u, inlier %u, error %.6g; two hand runs differ by %.3g, align() from the hand run by %.3g; %.4f m / %.5f rad from the truth\n",
                got.iterations, got.inlier, got.error, spread, diff, dt, da);
    CHECK(diff <= 4.0f * spread);
    CHECK(got.iterations >= 1 && got.iterations <= 6 && got.inlier > 300 && r.registration_result.converged);
    CHECK(r.registration_result.T.matrix() == pose_of(r.state));
}

// ------------------------------------------------------------------------------------------------ 3. the prior, golden pair
struct Golden {
    std::shared_ptr<PointCloudShared> source, target;
    alg::knn::KDTree::Ptr tree;
    M4 T_gt = M4::Identity();
};
static Golden& golden() {
    static Golden g;
    if (g.tree) return g;
    alg::filter::PreprocessFilter filter(*Q);
    alg::filter::VoxelGrid voxel(*Q, 0.25f);
    auto prep = [&](const std::string& name) {
        PointCloudShared scan(*Q, PointCloudReader::readFile(g_dir + "/" + name));
        filter.box_filter(scan, 0.5f, 50.0f);
        auto out = std::make_shared<PointCloudShared>(*Q);
        voxel.downsampling(scan, *out);
        with_covariances(*out, 10);
        return out;
    };
    g.source = prep("source.ply");
    g.target = prep("target.ply");
    g.tree = alg::knn::KDTree::build(*Q, *g.target);
    std::ifstream gt(g_dir + "/T_target_source.txt");
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) gt >> g.T_gt(r, c);
    std::printf("  golden pair: source %zu, target %zu points\n", g.source->size(), g.target->size());
    return g;
}

static void loose_prior() {
    Golden& g = golden();
    const imu::State pred = predicted(moved(g.T_gt));
    reg::RegistrationFactorParams factor;
    lio::LIORegistrationParams params;
    params.total_iterations = 10;
    params.optimization.optimization_method = reg::OptimizationMethod::LEVENBERG_MARQUARDT;
    params.directional_icp_weighting.enable = false;
    reg::RegistrationParams rp(factor, params.optimization);
    rp.max_iterations = 10;
    reg::Registration registration(*Q, rp);
    const auto ref = registration.align(*g.source, *g.target, *g.tree, pose_of(pred));
    const M15 P = diag15(1e6f);
    lio::LIORegistration lio_reg(*Q, factor, params);
    const auto r = lio_reg.align(*g.source, *g.target, *g.tree, pred, P, P, true, 0.1f, M4::Identity());
    float lt, la, rt, ra;
    pose_error(pose_of(r.state), g.T_gt, &lt, &la);
    pose_error(ref.T.matrix(), g.T_gt, &rt, &ra);
    std::printf("  loose prior (LM): LIO %.5f m / %.5f rad in %zu iterations; Registration::align %.5f m / %.5f rad in %zu\n", lt, la,
                r.registration_result.iterations, rt, ra, ref.iterations);
    CHECK(lt <= 2.0f * rt && la <= 2.0f * ra);
}

static void tight_prior() {
    Golden& g = golden();
    const imu::State pred = predicted(moved(g.T_gt));
    reg::RegistrationFactorParams factor;
    reg::Registration registration(*Q, reg::RegistrationParams(factor));
    const M4 T0 = pose_of(pred);
    const reg::LinearizedResult lin = registration.compute_linearized_result(*g.source, *g.target, *g.tree, T0, T0);
    double hf = 0.0, bn = 0.0;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < 6; ++j) hf += double(lin.H(i, j)) * double(lin.H(i, j));
        bn += double(lin.b(i)) * double(lin.b(i));
    }
    hf = std::sqrt(hf);
    bn = std::sqrt(bn);
    const M15 P = diag15(float(1.0 / (101.0 * hf)));
    const double h = 1.0 / double(P(0, 0));
    CHECK(h >= 100.0 * hf);
    const double bound = 2.0 * bn / h;
    lio::LIORegistrationParams params;
    params.total_iterations = 10;
    params.optimization.optimization_method = reg::OptimizationMethod::LEVENBERG_MARQUARDT;
    lio::LIORegistration lio_reg(*Q, factor, params);
    const auto r = lio_reg.align(*g.source, *g.target, *g.tree, pred, P, P, true, 0.1f, M4::Identity());
    float dp, da;
    pose_error(pose_of(r.state), T0, &dp, &da);
    std::printf("  tight prior (LM): |H_icp|_F %.4g, h %.4g, |b_icp| %.4g; |p - p_pred| %.3g m, angle %.3g rad, bound %.3g\n", hf, h, bn, dp,
                da, bound);
    CHECK(dp <= bound && da <= bound);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <golden dir>\n", argv[0]); return 2; }
    g_dir = argv[1];
    sycl_utils::DeviceQueue queue(0);
    Q = &queue;
    RUN(known_answers_lio);
    RUN(known_answers_imu);
    RUN(align_is_the_stepper_chain);
    RUN(loose_prior);
    RUN(tight_prior);
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
