// Loop closure: "have I been here before, and at what heading?" A database of Scan Context descriptors holds the keyframes so far
// (here: the bundled target scan between two decoys made from it, mirrored and stretched); the query is the bundled source scan
// turned by a further 150 degrees about z around its sensor, as if the place were revisited on the way back. The search compares
// the query with every entry under every column shift; the best candidate's shift is a yaw estimate, and its five initial guesses
// go through Registration::align_batch and best_of.
// usage: example_loop_closure <source.ply> <target.ply> [T_target_source.txt]
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
#include "sycl_points/amd/place_recognition.hpp"
#include "sycl_points/io/point_cloud_reader.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s source.ply target.ply [T_target_source.txt]\n", argv[0]); return 2; }
    using namespace sycl_points;
    namespace alg = sycl_points::algorithms;
    namespace reg = sycl_points::algorithms::registration;
    namespace pr = sycl_points::algorithms::place_recognition;
    sycl_utils::DeviceQueue queue(0);
    TransformMatrix turn = TransformMatrix::Identity();
    const float a = 150.0f * 3.14159265f / 180.0f;
    turn(0, 0) = std::cos(a); turn(0, 1) = -std::sin(a); turn(1, 0) = std::sin(a); turn(1, 1) = std::cos(a);

    // the raw scans: the descriptor wants the whole scan, the alignment a voxel-downsampled one
    PointCloudShared source(queue, PointCloudReader::readFile(argv[1])), target(queue, PointCloudReader::readFile(argv[2]));
    alg::transform::transform(source, turn);  // (about the sensor: the origin stays the sensor)
    PointCloudShared mirrored(target), stretched(target);
    TransformMatrix M = TransformMatrix::Identity(), S = TransformMatrix::Identity();
    M(1, 1) = -1.0f;
    S(0, 0) = S(1, 1) = 1.5f;
    alg::transform::transform(mirrored, M);
    alg::transform::transform(stretched, S);

    pr::ScanContextDatabase database(queue);
    database.add(stretched);
    const size_t target_index = database.add(target);
    database.add(mirrored);
    (void)database.query(source, 3);  // (loads the kernels)
    const auto t0 = std::chrono::steady_clock::now();
    const auto candidates = database.query(source, 3);
    const auto t1 = std::chrono::steady_clock::now();
    std::printf("%zu keyframes, query of %zu points: %.1f us (descriptor, search, read-back)\n", database.size(), source.size(),
                std::chrono::duration<double, std::micro>(t1 - t0).count());
    for (const auto& c : candidates)
        std::printf("  keyframe %d: distance %.4f at shift %d (yaw %.1f deg)%s\n", c.index, c.distance, c.shift, c.yaw * 180.0 / M_PI,
                    size_t(c.index) == target_index ? "  <- the place" : "");
    if (candidates.empty() || size_t(candidates[0].index) != target_index) { std::printf("the place was not recognised\n"); return 1; }

    // align the query to the recognised keyframe from the candidate's yaw
    alg::filter::PreprocessFilter filter(queue);
    alg::filter::VoxelGrid voxel(queue, 1.0f);
    auto prepare = [&](PointCloudShared& scan) {
        filter.box_filter(scan, 0.5f, 50.0f);
        auto out = std::make_shared<PointCloudShared>(queue);
        voxel.downsampling(scan, *out);
        const auto tree = alg::knn::KDTree::build(queue, *out);
        alg::covariance::estimate_async(tree->knn_search(*out, 20), *out).wait_and_throw();
        return out;
    };
    const auto src = prepare(source), tgt = prepare(target);
    const auto grid = alg::knn::GridKNN::build(queue, *tgt);
    reg::RegistrationParams params;
    params.reg_type = reg::RegType::GICP;
    params.max_correspondence_distance = 2.0f;
    params.max_iterations = 30;
    reg::Registration registration(queue, params);
    const auto from_identity = registration.align(*src, *tgt, *grid);
    const auto guesses = pr::initial_guesses(candidates[0], 5);
    const auto results = registration.align_batch(*src, *tgt, *grid, guesses);
    const size_t best = reg::Registration::best_of(results);
    if (best >= results.size()) { std::printf("no guess qualifies\n"); return 1; }
    const TransformMatrix T = results[best].T.matrix();
    std::printf("T_keyframe_query (guess %zu of %zu, %u inliers) =\n", best, guesses.size(), results[best].inlier);
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
        std::printf("against %s with the turn: align from the identity %.3f m, rotation (Frobenius) %.4f; from the loop candidate %.4f m, %.5f\n",
                    argv[3], it, ir, dt, dr);
        return dt < 0.2f && dr < 0.03f ? 0 : 1;
    }
    return 0;
}
