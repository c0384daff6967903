// Relocalisation against a VoxelHashMap: the target scan is accumulated into a map of 1 m voxels, the pose of the source scan is
// unknown, and Registration::align_batch(source, map, guesses) aligns it from a yaw sweep of 36 guesses in one launch, a workgroup
// per guess; best_of picks the hypothesis with the most inliers. Both scans are prepared as the reference's example prepares
// them (box filter [0.5, 50], voxel grid 0.25, k = 10 covariances); LM + GICP + Geman-McClure, 7 probed cells.
// usage: example_voxel_relocalization <source.ply> <target.ply> [T_target_source.txt]
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/filter/voxel_downsampling.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/mapping/voxel_hash_map.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s source.ply target.ply [T_target_source.txt]\n", argv[0]); return 2; }
    using namespace sycl_points;
    namespace alg = sycl_points::algorithms;
    namespace reg = sycl_points::algorithms::registration;
    sycl_utils::DeviceQueue queue(0);
    alg::filter::PreprocessFilter filter(queue);
    alg::filter::VoxelGrid voxel(queue, 0.25f);
    auto prepare = [&](const char* path) {
        PointCloudShared scan(queue, PointCloudReader::readFile(path));
        filter.box_filter(scan, 0.5f, 50.0f);
        auto out = std::make_shared<PointCloudShared>(queue);
        voxel.downsampling(scan, *out);
        const auto tree = alg::knn::KDTree::build(queue, *out);
        alg::covariance::estimate_async(tree->knn_search(*out, 10), *out).wait_and_throw();
        return out;
    };
    const auto source = prepare(argv[1]), target = prepare(argv[2]);

    alg::mapping::VoxelHashMap map(queue, 1.0f);
    map.add_point_cloud(*target, Eigen::Isometry3f::Identity());

    reg::RegistrationParams params;
    params.reg_type = reg::RegType::GICP;
    params.optimization_method = reg::OptimizationMethod::LEVENBERG_MARQUARDT;
    params.robust.type = alg::robust::RobustLossType::GEMAN_MCCLURE;
    params.robust.default_scale = 2.5f;
    params.max_correspondence_distance = 2.0f;
    params.max_iterations = 30;
    reg::Registration registration(queue, params);
    registration.set_voxel_neighbors(7);

    std::vector<TransformMatrix> guesses;
    for (int k = 0; k < 36; ++k) {  // the position is known roughly (the origin), the heading not at all
        const float a = 10.0f * k * 3.14159265f / 180.0f;
        TransformMatrix T = TransformMatrix::Identity();
        T(0, 0) = std::cos(a); T(0, 1) = -std::sin(a); T(1, 0) = std::sin(a); T(1, 1) = std::cos(a);
        guesses.push_back(T);
    }
    (void)registration.align_batch(*source, map, guesses);  // (prepares the map's registration rows, loads the kernels)
    const auto t0 = std::chrono::steady_clock::now();
    const auto results = registration.align_batch(*source, map, guesses);
    const auto t1 = std::chrono::steady_clock::now();
    const size_t best = reg::Registration::best_of(results);
    std::printf("source %zu points, target %zu points in 1 m voxels, %zu guesses in %.1f us\n", source->size(), target->size(),
                guesses.size(), std::chrono::duration<double, std::micro>(t1 - t0).count());
    for (size_t k = 0; k < results.size(); ++k)
        std::printf("  yaw %3zu deg: %2zu iterations, converged %d, inliers %5u, error %.6g%s\n", 10 * k, results[k].iterations,
                    int(results[k].converged), results[k].inlier, results[k].error, k == best ? "   <- best_of" : "");
    if (best >= results.size()) { std::printf("no hypothesis qualifies\n"); return 1; }
    const TransformMatrix T = results[best].T.matrix();
    std::printf("T_target_source (best_of) =\n");
    for (int r = 0; r < 4; ++r) std::printf("  % .6f % .6f % .6f % .6f\n", T(r, 0), T(r, 1), T(r, 2), T(r, 3));
    if (argc > 3) {
        std::ifstream f(argv[3]);
        TransformMatrix G = TransformMatrix::Identity();
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) f >> G(r, c);
        if (!f) { std::printf("cannot read %s\n", argv[3]); return 2; }
        float dt = 0.0f, dr = 0.0f;
        for (int r = 0; r < 3; ++r) {
            dt += (T(r, 3) - G(r, 3)) * (T(r, 3) - G(r, 3));
            for (int c = 0; c < 3; ++c) dr += (T(r, c) - G(r, c)) * (T(r, c) - G(r, c));
        }
        std::printf("against %s: translation %.4f m, rotation (Frobenius) %.5f\n", argv[3], std::sqrt(dt), std::sqrt(dr));
        return std::sqrt(dt) < 0.1f && std::sqrt(dr) < 0.02f ? 0 : 1;
    }
    return 0;
}
