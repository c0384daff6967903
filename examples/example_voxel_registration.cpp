// Voxelised GICP on the facade: the target scan is accumulated into a VoxelHashMap of 1 m voxels, as an odometry loop keeps its
// submap, and the source scan is aligned against the map itself with Registration::align(source, map) — no export of the voxel
// means, no tree on them, no covariance estimation for the target. Both scans are prepared as the reference's example prepares them
// (box filter [0.5, 50], voxel grid 0.25, k = 10 covariances); LM + GICP + Geman-McClure, from the identity.
// usage: example_voxel_registration <source.ply> <target.ply> [1 | 7 | 27 probed cells]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "sycl_points/algorithms/feature/covariance.hpp"
#include "sycl_points/algorithms/filter/preprocess_filter.hpp"
#include "sycl_points/algorithms/filter/voxel_downsampling.hpp"
#include "sycl_points/algorithms/knn/kdtree.hpp"
#include "sycl_points/algorithms/mapping/voxel_hash_map.hpp"
#include "sycl_points/algorithms/registration/registration.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s source.ply target.ply [1 | 7 | 27]\n", argv[0]); return 2; }
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
    params.max_iterations = 30;
    reg::Registration registration(queue, params);
    if (argc > 3) registration.set_voxel_neighbors(std::atoi(argv[3]));

    const auto t0 = std::chrono::steady_clock::now();
    const auto result = registration.align(*source, map);  // prepares the map's registration rows: the map has changed since
    const auto t1 = std::chrono::steady_clock::now();
    const auto again = registration.align(*source, map);   // the rows are still those of the map: nothing to refresh
    const auto t2 = std::chrono::steady_clock::now();
    std::printf("source %zu points, target %zu points in 1 m voxels, %d probed cells\n", source->size(), target->size(),
                registration.voxel_neighbors());
    std::printf("align: %.1f us with the rows prepared, %.1f us on the prepared map; %zu iterations, converged %d, inliers %u, error %.6g\n",
                std::chrono::duration<double, std::micro>(t1 - t0).count(), std::chrono::duration<double, std::micro>(t2 - t1).count(),
                result.iterations, int(result.converged), result.inlier, result.error);
    const TransformMatrix T = result.T.matrix();
    std::printf("T_target_source =\n");
    for (int r = 0; r < 4; ++r) std::printf("  % .6f % .6f % .6f % .6f\n", T(r, 0), T(r, 1), T(r, 2), T(r, 3));
    return std::memcmp(again.T.matrix().data(), T.data(), 16 * sizeof(float)) == 0 ? 0 : 1;
}
