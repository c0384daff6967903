// C++ test of the photometric term through the reference's include paths: feature::compute_intensity_gradients_async and the
// Registration::align overload that takes the target's gradients. Built and run by tests/test_gpu_photometric.py on a GPU box:
// test_photometric <scene file> <yardstick translation error> <yardstick rotation error>; exit code 0 = all checks passed.
// The scene file (written by that test, the textured plane of tests/f64_photometric.py): int32 n_source, n_target | then for the
// source and for the target: points (4 floats each), normals (4 floats each), intensities (1 float each). The pose that aligns
// them is yaw 2 degrees, t = (0.3, -0.2, 0.05); the yardsticks are the errors of the float64 aligner on the same clouds.
//   gradients     rows of the facade = rows of the C ABI call on the same buffers, bit for bit; the row count is remembered
//   weight_zero   the overload with weight 0 returns the bytes of the overload without gradients; the pose stays > 0.3 m off in the plane
//   optimizers    weight 25 under GAUSS_NEWTON, LEVENBERG_MARQUARDT, POWELL_DOGLEG: converged, errors within 3 x the yardsticks
//   degenerate    the same with the degenerate regulariser on (it sees the combined system)
//   error_paths   no source intensities, a size mismatch, a communicator set: each throws
// Every result is printed as "R <name> <in-plane error> <translation error> <rotation error> <converged> <iterations>".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"

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
static void section(const char* name, int failed_before) { std::printf("[ %s ] %s\n", g_failed == failed_before ? " OK " : "FAIL", name); }

static PointCloudCPU read_cloud(std::ifstream& f, int n) {
    PointCloudCPU c;
    c.points->resize(n);
    c.normals->resize(n);
    c.intensities->resize(n);
    f.read(reinterpret_cast<char*>(c.points->data()), sizeof(float) * 4 * n);
    f.read(reinterpret_cast<char*>(c.normals->data()), sizeof(float) * 4 * n);
    f.read(reinterpret_cast<char*>(c.intensities->data()), sizeof(float) * n);
    return c;
}
static M4 true_pose() {
    const double yaw = 2.0 * M_PI / 180.0;
    M4 T = M4::Identity();
    T(0, 0) = float(std::cos(yaw)); T(0, 1) = float(-std::sin(yaw));
    T(1, 0) = float(std::sin(yaw)); T(1, 1) = float(std::cos(yaw));
    T(0, 3) = 0.3f; T(1, 3) = -0.2f; T(2, 3) = 0.05f;
    return T;
}
struct Errors { double in_plane, trans, rot; };
static Errors errors_of(const M4& T) {
    const M4 want = true_pose();
    double t2 = 0.0, r2 = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double d = double(T(i, 3)) - double(want(i, 3));
        t2 += d * d;
        for (int j = 0; j < 3; ++j) r2 += (double(T(i, j)) - double(want(i, j))) * (double(T(i, j)) - double(want(i, j)));
    }
    return {std::hypot(double(T(0, 3)) - double(want(0, 3)), double(T(1, 3)) - double(want(1, 3))), std::sqrt(t2), std::sqrt(r2)};
}
static Errors report(const char* name, const reg::RegistrationResult& r) {
    const Errors e = errors_of(r.T.matrix());
    std::printf("R %s %.6e %.6e %.6e %d %zu\n", name, e.in_plane, e.trans, e.rot, int(r.converged), r.iterations);
    return e;
}
static reg::RegistrationParams params(float weight, reg::OptimizationMethod method) {
    reg::RegistrationParams p;
    p.reg_type = reg::RegType::POINT_TO_PLANE;
    p.max_correspondence_distance = 1.5f;
    p.max_iterations = 30;
    p.optimization_method = method;
    p.photometric.weight = weight;  // (everything else the defaults: criteria 1e-3)
    return p;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::printf("usage: %s <scene file> <translation yardstick> <rotation yardstick>\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    const double yard_t = std::stod(argv[2]), yard_r = std::stod(argv[3]);
    int32_t n[2] = {0, 0};
    f.read(reinterpret_cast<char*>(n), sizeof n);
    if (!f || n[0] <= 0 || n[1] <= 0) { std::printf("cannot read %s\n", argv[1]); return 2; }
    sycl_utils::DeviceQueue queue(0);
    const PointCloudCPU src = read_cloud(f, n[0]), tgt = read_cloud(f, n[1]);
    if (!f) { std::printf("%s is too short\n", argv[1]); return 2; }
    const PointCloudShared source(queue, src), target(queue, tgt);
    const auto tree = alg::knn::KDTree::build(queue, target);
    const auto neighbors = tree->knn_search(target, 10);
    std::printf("  source %zu points, target %zu points, yardsticks %.3e m / %.3e\n", source.size(), target.size(), yard_t, yard_r);

    int before = g_failed;
    const auto gradients = alg::feature::compute_intensity_gradients(neighbors, target);
    {
        CHECK(gradients.size() == target.size() && gradients.device_data() != nullptr);
        std::vector<float> a(4 * target.size()), b(4 * target.size(), -1.0f);
        float* raw = nullptr;
        hip_check(hipMalloc(&raw, b.size() * sizeof(float)), "hipMalloc");
        throw_on_error(sp_intensity_gradient(target.points_device(), target.normals_device(), target.intensities->device_data(), target.size(),
                                             neighbors.indices->device_data(), neighbors.k, raw, queue.stream()));
        hip_check(hipMemcpy(b.data(), raw, b.size() * sizeof(float), hipMemcpyDeviceToHost), "D2H");
        hip_check(hipMemcpy(a.data(), gradients.device_data(), a.size() * sizeof(float), hipMemcpyDeviceToHost), "D2H");
        (void)hipFree(raw);
        CHECK(std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
        size_t invalid = 0;
        for (size_t i = 0; i < target.size(); ++i) invalid += std::isnan(a[4 * i + 3]);
        CHECK(invalid == 0);
        PointCloudCPU bare;
        *bare.points = *tgt.points;
        const PointCloudShared no_attributes(queue, bare);
        bool threw = false;
        try { alg::feature::compute_intensity_gradients_async(neighbors, no_attributes); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
    }
    section("gradients", before);

    before = g_failed;
    {
        reg::Registration plain(queue, params(0.0f, reg::OptimizationMethod::GAUSS_NEWTON)), over(queue, params(0.0f, reg::OptimizationMethod::GAUSS_NEWTON));
        const auto a = plain.align(source, target, *tree);
        const auto b = over.align(source, target, *tree, gradients);
        CHECK(std::memcmp(a.T.matrix().data(), b.T.matrix().data(), 64) == 0 && a.iterations == b.iterations && a.inlier == b.inlier &&
              a.error == b.error && a.H == b.H && a.b == b.b);
        const Errors e = report("weight_zero", b);
        CHECK(e.in_plane > 0.3);
    }
    section("weight_zero", before);

    before = g_failed;
    {
        const std::pair<const char*, reg::OptimizationMethod> methods[] = {{"gauss_newton", reg::OptimizationMethod::GAUSS_NEWTON},
                                                                           {"levenberg_marquardt", reg::OptimizationMethod::LEVENBERG_MARQUARDT},
                                                                           {"powell_dogleg", reg::OptimizationMethod::POWELL_DOGLEG}};
        for (const auto& [name, method] : methods) {
            reg::Registration r(queue, params(25.0f, method));
            const auto res = r.align(source, target, *tree, gradients);
            const Errors e = report(name, res);
            CHECK(res.converged);
            CHECK(e.trans <= 3.0 * yard_t);
            CHECK(e.rot <= 3.0 * yard_r);
            CHECK(res.inlier > 0 && res.inlier <= source.size());
        }
    }
    section("optimizers", before);

    before = g_failed;
    {
        auto p = params(25.0f, reg::OptimizationMethod::GAUSS_NEWTON);
        p.degenerate_reg.type = reg::DegenerateRegularizationType::nl_reg;
        // a tenth of the default thresholds (10 / 1 per inlier, set for geometric factors): geometry alone is still held at the initial
        // pose (the plane's free directions have eigenvalue 0), the combined system (0.6 .. 1.9 per inlier in the plane) is not
        p.degenerate_reg.rot_eigenvalue_threshold = 1.0f;
        p.degenerate_reg.trans_eigenvalue_threshold = 0.1f;
        reg::Registration r(queue, p);
        const auto res = r.align(source, target, *tree, gradients);
        const Errors e = report("degenerate_reg", res);
        CHECK(res.converged && e.trans <= 3.0 * yard_t && e.rot <= 3.0 * yard_r);
        p.photometric.weight = 0.0f;
        reg::Registration alone(queue, p);
        CHECK(report("degenerate_reg_geometry_alone", alone.align(source, target, *tree, gradients)).in_plane > 0.3);
    }
    section("degenerate", before);

    before = g_failed;
    {
        reg::Registration r(queue, params(25.0f, reg::OptimizationMethod::GAUSS_NEWTON));
        PointCloudCPU no_i = src;
        no_i.intensities = std::make_shared<IntensityContainerCPU>();
        const PointCloudShared source_no_i(queue, no_i);
        bool threw = false;
        try { r.align(source_no_i, target, *tree, gradients); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
        alg::feature::IntensityGradients fewer = gradients;
        fewer.count = gradients.count - 1;
        threw = false;
        try { r.align(source, target, *tree, fewer); } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw);
        r.set_communicator(reinterpret_cast<sp_comm*>(uintptr_t(16)));  // (never dereferenced: the overload refuses first)
        threw = false;
        try { r.align(source, target, *tree, gradients); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
        r.set_communicator(nullptr);
        CHECK(r.align(source, target, *tree, gradients).converged);  // (and the object is still usable)
    }
    section("error_paths", before);

    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
