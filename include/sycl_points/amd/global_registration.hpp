// sycl_points facade for MI355X — global registration (MI355X extension; the reference has nothing of the kind).
//   registration::match_features            mutual nearest neighbours of two clouds' FPFH rows (sp_feature_match_mutual)
//   registration::GlobalRegistrationParams  how many triplet hypotheses are scored, how many become initial guesses, the gates
//   registration::global_guesses            match -> score -> select: the initial guesses Registration::align_global hands to
//                                           align_batch (registration.hpp)
// The descriptors come from feature::compute_fpfh_async (features.hpp) and need consistently oriented normals.
#pragma once
#include <cstdint>
#include <vector>

#include "features.hpp"

namespace sycl_points {
namespace algorithms {
namespace registration {

/// (i, j) pairs: source row i and target row j are each other's nearest neighbour in descriptor space; ascending in i.
struct FeatureMatches {
    shared_vector_ptr<int32_t> pairs = nullptr;  // 2 * count entries
    size_t count = 0;
    size_t size() const { return count; }
};

/// sp_feature_match_mutual on `queue`'s stream; one read-back (the count).
inline FeatureMatches match_features(const sycl_utils::DeviceQueue& queue, const feature::FPFHFeatures& source,
                                     const feature::FPFHFeatures& target) {
    FeatureMatches out;
    out.pairs = std::make_shared<shared_vector<int32_t>>(queue);
    const size_t ns = source.size(), nt = target.size();
    if (ns == 0 || nt == 0) return out;
    hipStream_t st = queue.stream();
    detail::DeviceScratch ws(sp_feature_match_mutual_workspace_bytes(ns, nt), st);
    uint32_t count = 0;
    int32_t* pairs = out.pairs->device_data_for_write(2 * std::min(ns, nt));
    throw_on_error(sp_feature_match_mutual(source.device_data(), ns, target.device_data(), nt, pairs, &count, ws.p, ws.bytes, st));
    out.count = count;
    out.pairs->set_device_size(2 * out.count);
    return out;
}

struct GlobalRegistrationParams {
    size_t hypotheses = 50000;     // triplets drawn and scored
    size_t guesses = 64;           // the best of them become align_batch's initial guesses
    float inlier_distance = 1.0f;  // a match counts for a hypothesis when its residual is below this
    float min_edge = 0.0f;         // every source edge of a triplet must be longer
    float edge_ratio = 0.9f;       // the shorter of two matching edges against the longer
    uint64_t seed = 0;             // of the counter-based triplet generator: the same seed, the same guesses
};

/// The initial guesses of a global registration: the poses of the params.guesses best-scoring matched triplets, best first (ties
/// to the lower hypothesis). Empty when fewer than three matches survive or no hypothesis passes its gates. Read-backs: the
/// match count; then the scores (4 bytes a hypothesis) and the matched points (32 bytes a match).
inline std::vector<TransformMatrix> global_guesses(const PointCloudShared& source, const feature::FPFHFeatures& source_features,
                                                   const PointCloudShared& target, const feature::FPFHFeatures& target_features,
                                                   const GlobalRegistrationParams& params, std::vector<uint32_t>* hypotheses_out = nullptr,
                                                   size_t* matches_out = nullptr) {
    std::vector<TransformMatrix> guesses;
    if (hypotheses_out) hypotheses_out->clear();
    if (matches_out) *matches_out = 0;
    if (source.size() == 0 || target.size() == 0 || params.hypotheses == 0 || params.guesses == 0) return guesses;
    if (source_features.size() != source.size() || target_features.size() != target.size())
        throw std::invalid_argument("[registration::global_guesses] one descriptor row per point is required");
    const sycl_utils::DeviceQueue& queue = source.queue;
    hipStream_t st = queue.stream();
    const FeatureMatches matches = match_features(queue, source_features, target_features);
    const size_t M = matches.size(), H = params.hypotheses;
    if (matches_out) *matches_out = M;
    if (M < 3) return guesses;
    detail::DeviceScratch dev(2 * M * 16 + H * 4, st);
    float* cs = static_cast<float*>(dev.p);
    float* ct = cs + 4 * M;
    uint32_t* score = reinterpret_cast<uint32_t*>(ct + 4 * M);
    throw_on_error(sp_correspondence_points(source.points_device(), source.size(), target.points_device(), target.size(),
                                            matches.pairs->device_data(), M, cs, ct, st));
    throw_on_error(sp_ransac_score(cs, ct, M, H, params.seed, params.inlier_distance, params.min_edge, params.edge_ratio, score, st));
    std::vector<float> host(8 * M + H);  // cs | ct | scores, as they lie on the device
    hip_check(hipMemcpyAsync(host.data(), dev.p, host.size() * 4, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    std::vector<double> poses(16 * params.guesses);
    std::vector<uint32_t> hyp(params.guesses);
    size_t count = 0;
    throw_on_error(sp_ransac_select_host(reinterpret_cast<const uint32_t*>(host.data() + 8 * M), H, host.data(), host.data() + 4 * M, M,
                                         params.seed, params.guesses, poses.data(), hyp.data(), &count));
    guesses.resize(count);
    for (size_t g = 0; g < count; ++g)
        for (int i = 0; i < 16; ++i) guesses[g].data()[i] = static_cast<float>(poses[16 * g + i]);
    if (hypotheses_out) hypotheses_out->assign(hyp.begin(), hyp.begin() + count);
    return guesses;
}

}  // namespace registration
}  // namespace algorithms
}  // namespace sycl_points
