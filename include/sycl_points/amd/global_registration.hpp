// sycl_points facade for MI355X — global registration (MI355X extension; the reference has nothing of the kind).
//   registration::match_features            mutual nearest neighbours of two clouds' FPFH rows (sp_feature_match_mutual)
//   registration::GlobalRegistrationParams  how many triplet hypotheses are scored, how many become initial guesses, the gates
//   registration::global_guesses            match -> score -> select: the initial guesses Registration::align_global hands to
//                                           align_batch (registration.hpp); params.method chooses between matched triplets and
//                                           the compatibility graph of DESIGN.md 4.22 (sp_compat_seeds .. sp_compat_select_host)
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

/// sp_feature_match on `queue`'s stream: every source row i with its nearest target row, as pairs (i, j) in ascending i. Unlike
/// the mutual matches these keep the inliers whose way back goes elsewhere; the compatibility graph sorts out the rest. One
/// read-back (the indices) and one upload (the pairs).
inline FeatureMatches match_features_nearest(const sycl_utils::DeviceQueue& queue, const feature::FPFHFeatures& source,
                                             const feature::FPFHFeatures& target) {
    FeatureMatches out;
    out.pairs = std::make_shared<shared_vector<int32_t>>(queue);
    const size_t ns = source.size(), nt = target.size();
    if (ns == 0 || nt == 0) return out;
    hipStream_t st = queue.stream();
    detail::DeviceScratch ws(sp_feature_match_workspace_bytes(ns, nt) + 4 * ns, st);
    int32_t* idx = reinterpret_cast<int32_t*>(static_cast<char*>(ws.p) + sp_feature_match_workspace_bytes(ns, nt));
    throw_on_error(sp_feature_match(source.device_data(), ns, target.device_data(), nt, idx, nullptr, ws.p,
                                    sp_feature_match_workspace_bytes(ns, nt), st));
    std::vector<int32_t> host(ns), pairs(2 * ns);
    hip_check(hipMemcpyAsync(host.data(), idx, 4 * ns, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    for (size_t i = 0; i < ns; ++i) pairs[2 * i] = static_cast<int32_t>(i), pairs[2 * i + 1] = host[i];
    out.pairs->assign(pairs.data(), pairs.size());
    out.count = ns;
    return out;
}

enum class GlobalGuessMethod {
    TRIPLETS,       // poses of random matched triplets, scored by the matches they explain (sp_ransac_score)
    COMPATIBILITY,  // least-squares poses of the densest neighbourhoods of the matches' compatibility graph (sp_compat_seeds)
};

struct GlobalRegistrationParams {
    size_t hypotheses = 50000;     // triplets drawn and scored
    size_t guesses = 64;           // the best of them become align_batch's initial guesses
    float inlier_distance = 1.0f;  // a match counts for a hypothesis when its residual is below this
    float min_edge = 0.0f;         // every source edge of a triplet must be longer
    float edge_ratio = 0.9f;       // the shorter of two matching edges against the longer
    uint64_t seed = 0;             // of the counter-based triplet generator: the same seed, the same guesses
    GlobalGuessMethod method = GlobalGuessMethod::TRIPLETS;
    float compat_tau = 0.1f;       // COMPATIBILITY: two matches are compatible when their two distances differ by less (min_edge gates them too)
    size_t compat_seeds = 64;      // consensus sets tried (<= SP_COMPAT_MAX_SEEDS)
    size_t compat_k = 16;          // companions per consensus set (<= SP_COMPAT_MAX_K)
};

/// The compatibility-graph guesses from M matched pairs: seeds -> consensus sets -> poses in double on the host -> scores ->
/// the params.guesses best (ties to the earlier seed rank). Read-backs: the lists and the matched points; then the scores.
inline std::vector<TransformMatrix> compat_guesses_of_matches(const PointCloudShared& source, const PointCloudShared& target,
                                                   const FeatureMatches& matches, const GlobalRegistrationParams& params,
                                                   std::vector<uint32_t>* ranks_out) {
    std::vector<TransformMatrix> guesses;
    const size_t M = matches.size(), S = params.compat_seeds, K = params.compat_k;
    if (M < 3 || S == 0 || K == 0) return guesses;
    hipStream_t st = source.queue.stream();
    const size_t list_words = 2 * S + S * K;  // seed_idx | seed_s | consensus lists
    detail::DeviceScratch dev(2 * M * 16 + list_words * 4, st), ws(sp_compat_workspace_bytes(M), st);
    float* cs = static_cast<float*>(dev.p);
    float* ct = cs + 4 * M;
    int32_t* seed_idx = reinterpret_cast<int32_t*>(ct + 4 * M);
    uint32_t* seed_s = reinterpret_cast<uint32_t*>(seed_idx + S);
    int32_t* cons = seed_idx + 2 * S;
    throw_on_error(sp_correspondence_points(source.points_device(), source.size(), target.points_device(), target.size(),
                                            matches.pairs->device_data(), M, cs, ct, st));
    throw_on_error(sp_compat_seeds(cs, ct, M, params.compat_tau, params.min_edge, S, seed_idx, seed_s, nullptr, nullptr, ws.p, ws.bytes, st));
    throw_on_error(sp_compat_consensus(M, seed_idx, S, K, cons, nullptr, ws.p, ws.bytes, st));
    std::vector<float> host(8 * M + list_words);  // cs | ct | lists, as they lie on the device
    hip_check(hipMemcpyAsync(host.data(), dev.p, host.size() * 4, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    const int32_t* seed_idx_host = reinterpret_cast<const int32_t*>(host.data() + 8 * M);
    std::vector<double> poses(16 * S);
    std::vector<uint32_t> ranks(S);
    size_t count = 0;
    throw_on_error(sp_compat_poses_host(host.data(), host.data() + 4 * M, M, seed_idx_host, seed_idx_host + 2 * S, S, K, poses.data(),
                                        ranks.data(), &count));
    if (count == 0) return guesses;
    std::vector<float> poses_f(16 * count);
    for (size_t i = 0; i < poses_f.size(); ++i) poses_f[i] = static_cast<float>(poses[i]);
    detail::DeviceScratch pd(count * (64 + 4), st);
    uint32_t* score = reinterpret_cast<uint32_t*>(static_cast<float*>(pd.p) + 16 * count);
    hip_check(hipMemcpyAsync(pd.p, poses_f.data(), poses_f.size() * 4, hipMemcpyHostToDevice, st), "H2D");
    throw_on_error(sp_pose_score(cs, ct, M, static_cast<const float*>(pd.p), count, params.inlier_distance, score, st));
    std::vector<uint32_t> scores(count);
    hip_check(hipMemcpyAsync(scores.data(), score, count * 4, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    std::vector<double> best(16 * params.guesses);
    std::vector<uint32_t> best_rank(params.guesses);
    size_t kept = 0;
    throw_on_error(sp_compat_select_host(scores.data(), poses.data(), ranks.data(), count, params.guesses, best.data(), best_rank.data(), &kept));
    guesses.resize(kept);
    for (size_t g = 0; g < kept; ++g)
        for (int i = 0; i < 16; ++i) guesses[g].data()[i] = static_cast<float>(best[16 * g + i]);
    if (ranks_out) ranks_out->assign(best_rank.begin(), best_rank.begin() + kept);
    return guesses;
}

/// The initial guesses of a global registration: the poses of the params.guesses best-scoring matched triplets, best first (ties
/// to the lower hypothesis). Empty when fewer than three matches survive or no hypothesis passes its gates. Read-backs: the
/// match count; then the scores (4 bytes a hypothesis) and the matched points (32 bytes a match).
/// params.method == COMPATIBILITY: the matches are every source row with its nearest target row (match_features_nearest; the
/// mutual matches when the source has more than SP_COMPAT_MAX_MATCHES rows, nothing when those are too many as well), the
/// guesses compat_guesses_of_matches', best score first (ties to the earlier seed rank), and hypotheses_out the seed ranks.
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
    const bool compat = params.method == GlobalGuessMethod::COMPATIBILITY;
    const FeatureMatches matches = compat && source.size() <= SP_COMPAT_MAX_MATCHES
                                       ? match_features_nearest(queue, source_features, target_features)
                                       : match_features(queue, source_features, target_features);
    const size_t M = matches.size(), H = params.hypotheses;
    if (matches_out) *matches_out = M;
    if (M < 3) return guesses;
    if (compat) return M <= SP_COMPAT_MAX_MATCHES ? compat_guesses_of_matches(source, target, matches, params, hypotheses_out) : guesses;
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
