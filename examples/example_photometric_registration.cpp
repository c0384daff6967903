// The photometric term of Registration::align where geometry alone cannot fix the pose: a textured plane.
// Target: 3000 points uniform in [-6, 6]^2 on z = 0 with a smooth intensity pattern; source: 1500 other samples of the same surface,
// moved by the inverse of {yaw 2 degrees, t = (0.3, -0.2, 0.05) m}. Point-to-plane from the identity recovers z and nothing else;
// with target intensity gradients (feature::compute_intensity_gradients) and RegistrationParams::photometric.weight = 25 the pattern
// pins the other three degrees of freedom. Built in the program: no data file.
// usage: example_photometric_registration [weight=25]
#include <cmath>
#include <cstdio>
#include <random>
#include <string>

#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"

using namespace sycl_points;
namespace alg = sycl_points::algorithms;
namespace reg = sycl_points::algorithms::registration;

static float pattern(double x, double y) {
    return float(0.5 + 0.25 * std::sin(2 * M_PI * x / 4 + 0.3) + 0.25 * std::sin(2 * M_PI * y / 5 + 1.1) * std::cos(2 * M_PI * x / 7));
}
// n samples of the plane, then moved by the rigid motion (yaw, tx, ty, tz)
static PointCloudCPU textured_plane(size_t n, unsigned seed, double yaw, double tx, double ty, double tz) {
    std::mt19937 gen(seed);
    std::uniform_real_distribution<double> u(-6.0, 6.0);
    PointCloudCPU c;
    for (size_t i = 0; i < n; ++i) {
        const double x = u(gen), y = u(gen);
        c.points->push_back(PointType(float(std::cos(yaw) * x - std::sin(yaw) * y + tx), float(std::sin(yaw) * x + std::cos(yaw) * y + ty), float(tz), 1.0f));
        c.normals->push_back(Normal(0.0f, 0.0f, 1.0f, 0.0f));
        c.intensities->push_back(pattern(x, y));
    }
    return c;
}
static void print_pose(const char* what, const reg::RegistrationResult& r) {
    const auto& T = r.T.matrix();
    const double yaw = std::atan2(double(T(1, 0)), double(T(0, 0))) * 180.0 / M_PI;
    std::printf("%-28s t = (% .4f, % .4f, % .4f) m, yaw = % .4f deg, %s after %zu iterations, %u inliers\n", what, T(0, 3), T(1, 3), T(2, 3), yaw,
                r.converged ? "converged" : "NOT converged", r.iterations, r.inlier);
}

int main(int argc, char** argv) {
    const float weight = argc > 1 ? std::stof(argv[1]) : 25.0f;
    sycl_utils::DeviceQueue queue(0);
    const double yaw = 2.0 * M_PI / 180.0;
    // the source is the plane seen from a frame that T = {yaw, (0.3, -0.2, 0.05)} takes back onto the target: p_source = T^-1 p
    const double c = std::cos(-yaw), s = std::sin(-yaw);
    const double itx = -(c * 0.3 - s * -0.2), ity = -(s * 0.3 + c * -0.2), itz = -0.05;
    const PointCloudShared target(queue, textured_plane(3000, 1, 0.0, 0.0, 0.0, 0.0));
    const PointCloudShared source(queue, textured_plane(1500, 2, -yaw, itx, ity, itz));
    const auto tree = alg::knn::KDTree::build(queue, target);
    const auto gradients = alg::feature::compute_intensity_gradients(tree->knn_search(target, 10), target);

    reg::RegistrationParams p;
    p.reg_type = reg::RegType::POINT_TO_PLANE;
    p.max_correspondence_distance = 1.5f;
    p.max_iterations = 30;
    std::printf("truth                        t = ( 0.3000, -0.2000,  0.0500) m, yaw =  2.0000 deg\n");
    reg::Registration geometry(queue, p);
    print_pose("point-to-plane alone", geometry.align(source, target, *tree));
    p.photometric.weight = weight;
    reg::Registration both(queue, p);
    print_pose(("with the photometric term x" + std::to_string(int(weight))).c_str(), both.align(source, target, *tree, gradients));
    return 0;
}
