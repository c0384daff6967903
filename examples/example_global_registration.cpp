// Global registration: the pose of the source scan is unknown altogether (here: the bundled source turned by a further 150 degrees
// about z around its sensor), so no sweep of guesses is at hand. FPFH descriptors of both scans at 1 m voxels, their mutual nearest
// neighbours, 50 000 triplet hypotheses scored by the matches they explain, the 64 best as the initial guesses of align_batch, and
// best_of picks the winner: Registration::align_global. The descriptors need normals that all point towards the sensor:
// covariance::estimate_normals_async leaves a plane that passes within 1 m of the sensor as its eigenvector came out, so the
// example turns those itself.
// usage: example_global_registration <source.ply> <target.ply> [T_target_source.txt]
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include "sycl_points/algorithms/common/transform.hpp"
#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/filter/voxel_downsampling.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s source.ply target.ply [T_target_source.txt]\n", argv[0]); return 2; }
    using namespace sycl_points;
    namespace alg = sycl_points::algorithms;
    namespace reg = sycl_points::algorithms::registration;
    sycl_utils::DeviceQueue queue(0);
    alg::filter::PreprocessFilter filter(queue);
    alg::filter::VoxelGrid voxel(queue, 1.0f);
    TransformMatrix turn = TransformMatrix::Identity();
    const float a = 150.0f * 3.14159265f / 180.0f;
    turn(0, 0) = std::cos(a); turn(0, 1) = -std::sin(a); turn(1, 0) = std::sin(a); turn(1, 1) = std::cos(a);

    struct Prepared {
        std::shared_ptr<PointCloudShared> cloud;
        alg::feature::FPFHFeatures features;
    };
    auto prepare = [&](const char* path, const TransformMatrix* T) {
        PointCloudShared scan(queue, PointCloudReader::readFile(path));
        filter.box_filter(scan, 0.5f, 50.0f);
        Prepared out;
        out.cloud = std::make_shared<PointCloudShared>(queue);
        voxel.downsampling(scan, *out.cloud);
        if (T) alg::transform::transform(*out.cloud, *T);  // (a rotation about the sensor: the origin stays the sensor)
        const auto tree = alg::knn::KDTree::build(queue, *out.cloud);
        const auto neighbors = tree->knn_search(*out.cloud, 20);
        alg::covariance::estimate_async(neighbors, *out.cloud).wait_and_throw();
        alg::covariance::estimate_normals_async(tree->knn_search(*out.cloud, 10), *out.cloud).wait_and_throw();
        for (size_t i = 0; i < out.cloud->size(); ++i) {  // every normal towards the sensor
            const auto& p = (*out.cloud->points)[i];
            auto& n = (*out.cloud->normals)[i];
            if (n[0] * p[0] + n[1] * p[1] + n[2] * p[2] > 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        }
        out.features = alg::feature::compute_fpfh(neighbors, *out.cloud);
        return out;
    };
    const Prepared source = prepare(argv[1], &turn), target = prepare(argv[2], nullptr);
    const auto grid = alg::knn::GridKNN::build(queue, *target.cloud);

    reg::RegistrationParams params;
    params.reg_type = reg::RegType::GICP;
    params.max_correspondence_distance = 2.0f;
    params.max_iterations = 30;
    reg::Registration registration(queue, params);
    reg::GlobalRegistrationParams global;
    global.inlier_distance = 1.0f;
    global.seed = 2024;

    const auto from_identity = registration.align(*source.cloud, *target.cloud, *grid);
    std::vector<reg::RegistrationResult> all;
    (void)registration.align_global(*source.cloud, source.features, *target.cloud, target.features, *grid, global);  // (loads the kernels)
    const auto t0 = std::chrono::steady_clock::now();
    const auto result = registration.align_global(*source.cloud, source.features, *target.cloud, target.features, *grid, global, &all);
    const auto t1 = std::chrono::steady_clock::now();
    std::printf("source %zu points, target %zu points at 1 m voxels; %zu hypotheses, %zu guesses aligned, %.1f us\n", source.cloud->size(),
                target.cloud->size(), global.hypotheses, all.size(), std::chrono::duration<double, std::micro>(t1 - t0).count());
    if (!result.converged) { std::printf("no hypothesis qualifies\n"); return 1; }
    const TransformMatrix T = result.T.matrix();
    std::printf("T_target_source (align_global, %u inliers) =\n", result.inlier);
    for (int r = 0; r < 4; ++r) std::printf("  % .6f % .6f % .6f % .6f\n", T(r, 0), T(r, 1), T(r, 2), T(r, 3));
    if (argc > 3) {
        std::ifstream f(argv[3]);
        TransformMatrix G = TransformMatrix::Identity();
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) f >> G(r, c);
        if (!f) { std::printf("cannot read %s\n", argv[3]); return 2; }
        TransformMatrix back = turn;  // the inverse of a rotation about z: its transpose
        back(0, 1) = turn(1, 0); back(1, 0) = turn(0, 1);
        G = G * back;  // the source was turned: T_target_source . Rz(150)^-1
        auto errors = [&](const TransformMatrix& X, float& dt, float& dr) {
            dt = dr = 0.0f;
            for (int r = 0; r < 3; ++r) {
                dt += (X(r, 3) - G(r, 3)) * (X(r, 3) - G(r, 3));
                for (int c = 0; c < 3; ++c) dr += (X(r, c) - G(r, c)) * (X(r, c) - G(r, c));
            }
            dt = std::sqrt(dt), dr = std::sqrt(dr);
        };
        float dt, dr, it, ir;
        errors(T, dt, dr);
        errors(from_identity.T.matrix(), it, ir);
        std::printf("against %s with the turn: align from the identity %.3f m, rotation (Frobenius) %.4f; align_global %.4f m, %.5f\n", argv[3],
                    it, ir, dt, dr);
        return dt < 0.2f && dr < 0.03f ? 0 : 1;
    }
    return 0;
}
