// sycl_points facade for MI355X — registration layer.
//   algorithms/robust/robust.hpp                         : RobustLossType (+ from_string)
//   algorithms/registration/factor.hpp                   : RegType (+ from_string)
//   algorithms/registration/registration_params.hpp      : RegistrationParams and friends
//   algorithms/registration/{linearized_result,result}.hpp
//   algorithms/registration/registration.hpp             : Registration (align, compute_linearized_result,
//                                                          compute_error_frozen, compute_icp_robust_weights)
//   algorithms/deskew/relative_pose_deskew.hpp           : deskew::deskew_point_cloud_constant_velocity
//   algorithms/registration/pipeline/{aligner,velocity_update,robust}.hpp, registration_pipeline(_params).hpp
//   global_registration.hpp (no header of the reference) : match_features, GlobalRegistrationParams, global_guesses, behind
//                                                          Registration::align_global — MI355X extension
// Host control flow follows the reference; every per-point kernel is a C-ABI call. When the KNNBase handed to align()
// is a GridKNN and the factor is GICP, the iteration uses the prepared / fused kernel (sp_gicp_iteration_fused).
#pragma once
#include <cctype>
#include <cstring>
#include <functional>
#include <memory>
#include <optional>
#include <vector>
#include <iostream>
#include <tuple>

#include "features.hpp"
#include "global_registration.hpp"
#include "mapping.hpp"

namespace sycl_points {
namespace algorithms {

// robust::RobustLossType lives in features.hpp (covariance::estimate_robust_async needs it too)

// ------------------------------------------------------------------------------------------------ deskew
namespace deskew {

/// deskew/relative_pose_deskew.hpp:36-178 — constant body velocity between two poses: every point is moved from the sensor
/// frame at its own time stamp into the frame of `current_relative_pose`; normals and covariances are rotated with it. One
/// kernel (sp_deskew_constant_velocity), data stays on the device. In place (`&input_cloud == &output_cloud`) is allowed and —
/// unlike the reference, which zeroes its outputs before it reads its inputs — returns the rotated normals and covariances.
/// false: an empty cloud, a cloud without time stamps, a duration <= 0.
inline bool deskew_point_cloud_constant_velocity(const PointCloudShared& input_cloud, PointCloudShared& output_cloud,
                                                 const Eigen::Isometry3f& previous_relative_pose,
                                                 const Eigen::Isometry3f& current_relative_pose,
                                                 float inter_scan_duration_seconds = -1.0f) {
    if (!input_cloud.queue.ptr || !output_cloud.queue.ptr)
        throw std::runtime_error("[deskew_point_cloud_constant_velocity] SYCL queue is not initialized");
    const size_t N = input_cloud.size();
    if (N == 0 || !input_cloud.has_timestamps()) return false;
    const float duration = inter_scan_duration_seconds > 0.0f
                               ? inter_scan_duration_seconds
                               : static_cast<float>((input_cloud.end_time_ms - input_cloud.start_time_ms) * 1e-3);
    if (duration <= 0.0f) return false;
    float twist[6];
    sp_relative_twist_host(previous_relative_pose.matrix().data(), current_relative_pose.matrix().data(), twist);
    const sycl_points::detail::DeskewBuffers b = sycl_points::detail::prepare_deskew_output(input_cloud, output_cloud);  // :62-95
    throw_on_error(sp_deskew_constant_velocity(b.points_in, b.covs_in, b.normals_in, input_cloud.timestamp_offsets->device_data(), N,
                                               twist, duration, b.points_out, b.covs_out, b.normals_out, input_cloud.queue.stream()));
    sycl_utils::events(input_cloud.queue.stream()).wait_and_throw();  // :175
    return true;
}

}  // namespace deskew

namespace registration {

enum class RegType { POINT_TO_POINT = 0, POINT_TO_PLANE, POINT_TO_DISTRIBUTION, GICP, GENZ };  // factor.hpp:18-32
inline RegType RegType_from_string(const std::string& str) {
    std::string u = str;
    for (auto& c : u) c = (char)std::toupper((unsigned char)c);
    if (u == "POINT_TO_POINT") return RegType::POINT_TO_POINT;
    if (u == "POINT_TO_PLANE") return RegType::POINT_TO_PLANE;
    if (u == "GICP") return RegType::GICP;
    if (u == "GENZ") return RegType::GENZ;
    if (u == "POINT_TO_DISTRIBUTION" || u == "P2D") return RegType::POINT_TO_DISTRIBUTION;
    throw std::runtime_error("[RegType_from_string] Invalid RegType str '" + str + "'");
}
enum class OptimizationMethod { GAUSS_NEWTON = 0, LEVENBERG_MARQUARDT, POWELL_DOGLEG };
inline OptimizationMethod OptimizationMethod_from_string(const std::string& str) {
    std::string u = str;
    for (auto& c : u) c = (char)std::toupper((unsigned char)c);
    if (u == "GN" || u == "GAUSS_NEWTON") return OptimizationMethod::GAUSS_NEWTON;
    if (u == "LM" || u == "LEVENBERG_MARQUARDT") return OptimizationMethod::LEVENBERG_MARQUARDT;
    if (u == "DOGLEG" || u == "POWELL_DOGLEG") return OptimizationMethod::POWELL_DOGLEG;
    throw std::runtime_error("[OptimizationMethod_from_string] Invalid OptimizationMethod str [" + str + "]");
}

/// registration_params.hpp:41-114 (same fields, same defaults)
struct RegistrationConvergenceCriteria {
    float translation = 1e-3f;
    float rotation = 1e-3f;
};
struct RegistrationFactorParams {
    struct Robust { robust::RobustLossType type = robust::RobustLossType::NONE; float default_scale = 10.0f; };
    struct GenZ { float planarity_threshold = 0.2f; };
    struct RotationConstraint {  // registration_params.hpp:56-64
        struct Robust { float default_scale = 10.0f; };
        bool enable = false;
        float weight = 1.0f;
        Robust robust;
    };
    RegType reg_type = RegType::GICP;
    float max_correspondence_distance = 2.0f;
    Robust robust;
    RotationConstraint rotation_constraint;
    GenZ genz;
    bool verbose = false;
};
/// degenerate_regularization.hpp:14-46
enum class DegenerateRegularizationType { none = 0, nl_reg };
inline DegenerateRegularizationType DegenerateRegularizationType_from_string(const std::string& str) {
    std::string u = str;
    for (auto& c : u) c = (char)std::toupper((unsigned char)c);
    if (u == "NONE") return DegenerateRegularizationType::none;
    if (u == "NL-REG" || u == "NL_REG") return DegenerateRegularizationType::nl_reg;
    throw std::runtime_error("[DegenerateRegularizationType_from_string] Invalid DegenerateRegularizationType str [" + str + "]");
}
struct DegenerateRegularizationParams {
    DegenerateRegularizationType type = DegenerateRegularizationType::none;
    float rot_eigenvalue_threshold = 10.0f;
    float trans_eigenvalue_threshold = 1.0f;
    float base_factor = 1.0f;
};
/// map_prior.hpp:14-35
struct MapPriorParams {
    bool enabled = false;
    float rot_vel_sigma = 1.0f;
    float trans_vel_sigma = 1.0f;
    float rot_base_sigma = 3.16e-2f;
    float trans_base_sigma = 1e-2f;
};
/// MI355X extension (the reference has no such field): the photometric term of Registration::align's overload that takes the
/// target's feature::IntensityGradients. weight 0: off.
struct PhotometricParams {
    float weight = 0.0f;
    robust::RobustLossType robust_type = robust::RobustLossType::NONE;
    float robust_scale = 1.0f;
};
struct RegistrationOptimizationParams {
    struct GaussNewton { float lambda = 1.0f; };
    struct LevenbergMarquardt {
        size_t max_inner_iterations = 10;
        float lambda_factor = 2.0f, init_lambda = 1.0f, max_lambda = 1e3f, min_lambda = 1e-6f;
    };
    struct Dogleg {  // registration_params.hpp:84-92
        float initial_trust_region_radius = 1.0f, min_trust_region_radius = 1e-4f, max_trust_region_radius = 10.0f;
        float eta1 = 0.25f, eta2 = 0.75f, gamma_decrease = 0.25f, gamma_increase = 2.0f;
    };
    GaussNewton gn;
    LevenbergMarquardt lm;
    Dogleg dogleg;
    OptimizationMethod optimization_method = OptimizationMethod::GAUSS_NEWTON;
};
struct RegistrationParams : public RegistrationFactorParams, public RegistrationOptimizationParams {
    using Criteria = RegistrationConvergenceCriteria;
    RegistrationParams() = default;
    /// registration_params.hpp:104-107: from the two halves (what Parameters::make_registration_pipeline_params passes)
    explicit RegistrationParams(const RegistrationFactorParams& factor, const RegistrationOptimizationParams& optimization = {})
        : RegistrationFactorParams(factor), RegistrationOptimizationParams(optimization) {}
    size_t max_iterations = 20;
    Criteria criteria;
    DegenerateRegularizationParams degenerate_reg;  // registration_params.hpp:111-112
    MapPriorParams map_prior;
    PhotometricParams photometric;
};

/// linearized_result.hpp:12-24
struct LinearizedResult {
    Eigen::Matrix<float, 6, 6> H = Eigen::Matrix<float, 6, 6>::Zero();
    Eigen::Matrix<float, 6, 1> b = Eigen::Matrix<float, 6, 1>::Zero();
    float error = std::numeric_limits<float>::max();
    uint32_t inlier = 0;
};
/// result.hpp:12-28
struct RegistrationResult {
    using Ptr = std::shared_ptr<RegistrationResult>;
    Eigen::Isometry3f T = Eigen::Isometry3f::Identity();
    bool converged = false;
    size_t iterations = 0;
    Eigen::Matrix<float, 6, 6> H = Eigen::Matrix<float, 6, 6>::Zero();
    Eigen::Matrix<float, 6, 1> b = Eigen::Matrix<float, 6, 1>::Zero();
    float error = std::numeric_limits<float>::max();
    Eigen::Matrix<float, 6, 6> H_raw = Eigen::Matrix<float, 6, 6>::Zero();
    Eigen::Matrix<float, 6, 1> b_raw = Eigen::Matrix<float, 6, 1>::Zero();
    float error_raw = std::numeric_limits<float>::max();
    uint32_t inlier = 0;
};

/// registration.hpp:88-965
class Registration {
public:
    using Ptr = std::shared_ptr<Registration>;
    struct ExecutionOptions {  // registration.hpp:92-100
        float robust_scale;
        float rotation_robust_scale;
        float dt;
        TransformMatrix prev_pose;
        ExecutionOptions() : robust_scale(-1.0f), rotation_robust_scale(-1.0f), dt(0.1f), prev_pose(TransformMatrix::Identity()) {}
    };

    explicit Registration(const sycl_utils::DeviceQueue& queue, const RegistrationParams& params = RegistrationParams())
        : params_(params), queue_(queue) {
        hip_check(hipMalloc(&lin_dev_, sizeof(sp_linearized)), "hipMalloc");
        ws_bytes_ = sp_gicp_workspace_bytes(0);
        hip_check(hipMalloc(&ws_, ws_bytes_), "hipMalloc");
        hip_check(hipMalloc(&T_dev_, (16 + 8 + 4) * sizeof(float)), "hipMalloc");  // pose | delta[8] | iterations
        // read-backs (one 192-byte system or one error per optimiser step) land in pinned memory: a copy into pageable memory
        // is staged and blocks inside the runtime (2.24 -> 1.94 ms for the LM alignment of the reference's example)
        hip_check(hipHostMalloc(&pin_, 4096), "hipHostMalloc");
        hip_check(hipMalloc(&res_dev_, sizeof(sp_align_result)), "hipMalloc");
        // the device-resident optimiser's pose (64 bytes each way) and result block in host-mapped memory, when it is to be had:
        // the host writes the initial guess, the launch stores the block and then its `done` word, the host spins on that word —
        // no copy in, no copy out, no synchronisation
        void* m = nullptr;
        if (hipHostMalloc(&m, kMappedBytes, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess) {
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, m, 0) == hipSuccess) { map_host_ = static_cast<char*>(m); map_dev_ = static_cast<char*>(d); }
            else { (void)hipGetLastError(); (void)hipHostFree(m); }
        } else {
            (void)hipGetLastError();
        }
    }
    ~Registration() {
        if (psrc_) sp_gicp_source_destroy(psrc_);
        if (ptgt_) sp_gicp_target_destroy(ptgt_);
        (void)hipFree(lin_dev_); (void)hipFree(ws_); (void)hipFree(T_dev_); (void)hipFree(res_dev_);
        if (pin_) (void)hipHostFree(pin_);
        if (map_host_) (void)hipHostFree(map_host_);
        if (batch_dev_) (void)hipFree(batch_dev_);
        if (batch_pin_) (void)hipHostFree(batch_pin_);
        if (vws_) (void)hipFree(vws_);
    }
    Registration(const Registration&) = delete;
    Registration& operator=(const Registration&) = delete;

    /// registration.hpp:124-126 / MapPrior::update (map_prior.hpp:97-174): once per frame, after motion prediction and
    /// before align().
    void set_map_prior_state(const RegistrationResult& prev_result, const Eigen::Isometry3f& T_pred) {
        const sp_map_prior_params mp{params_.map_prior.enabled ? 1 : 0, params_.map_prior.rot_vel_sigma,
                                     params_.map_prior.trans_vel_sigma, params_.map_prior.rot_base_sigma,
                                     params_.map_prior.trans_base_sigma};
        float H36[36];
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) H36[i * 6 + j] = prev_result.H_raw(i, j);
        const TransformMatrix Tprev = prev_result.T.matrix(), Tpred = T_pred.matrix();
        throw_on_error(sp_map_prior_update_host(&mp, H36, prev_result.error_raw, prev_result.inlier, Tprev.data(),
                                                Tpred.data(), &map_prior_));
    }

    /// registration.hpp:129-193
    void validate_params(const PointCloudShared& source, const PointCloudShared& target, RegistrationParams& params) const {
        if (params.reg_type == RegType::POINT_TO_PLANE && !target.has_normal()) {
            if (!target.has_cov())
                throw std::runtime_error("[Registration::validate_params] Normal vector or covariance matrices of target "
                                         "must be pre-computed before performing Point-to-Plane ICP matching.");
            covariance::extract_normals(target);
        }
        if (params.reg_type == RegType::GICP && (!source.has_cov() || !target.has_cov()))
            throw std::runtime_error("[Registration::validate_params] Covariance matrices of source and target must be "
                                     "pre-computed before performing GICP matching.");
        if (params.reg_type == RegType::GENZ) {
            if (!target.has_cov())
                throw std::runtime_error("[Registration::validate_params] Covariance matrices of target must be "
                                         "pre-computed before performing GenZ-ICP matching.");
            if (!target.has_normal()) covariance::extract_normals(target);
        }
        if (params.reg_type == RegType::POINT_TO_DISTRIBUTION && !target.has_cov())
            throw std::runtime_error("[Registration::validate_params] Covariance matrices of target must be pre-computed "
                                     "before performing Point-to-Distribution ICP matching.");
        if (params.rotation_constraint.enable) {
            if (!source.has_cov())
                throw std::runtime_error("[Registration::validate_params] Covariance matrices of source are required for "
                                         "performing rotation constraint matching.");
            if (!target.has_cov())
                throw std::runtime_error("[Registration::validate_params] Covariance matrices of target are required for "
                                         "performing rotation constraint matching.");
        }
        if (params.robust.type != robust::RobustLossType::NONE && params.robust.default_scale <= 0.0f) {
            std::cout << "[Caution] `robust.default_scale` must be greater than zero. Disable robust loss." << std::endl;
            params.robust.type = robust::RobustLossType::NONE;
        }
    }

    /// registration.hpp:201-276
    RegistrationResult align(const PointCloudShared& source, const PointCloudShared& target, const knn::KNNBase& target_knn,
                             const TransformMatrix& initial_guess = TransformMatrix::Identity(),
                             const ExecutionOptions& options = ExecutionOptions()) {
        RegistrationResult result;
        result.T.matrix() = initial_guess;
        if (source.size() == 0) return result;
        validate_params(source, target, params_);
        const float robust_scale = options.robust_scale > 0.0f ? options.robust_scale : params_.robust.default_scale;
        rotation_robust_scale_ = options.rotation_robust_scale > 0.0f ? options.rotation_robust_scale
                                                                      : params_.rotation_constraint.robust.default_scale;
        const bool pose_terms = params_.degenerate_reg.type != DegenerateRegularizationType::none || prior_active();
        const auto* grid = dynamic_cast<const knn::GridKNN*>(&target_knn);
        // A caller that still hands over the reference's KDTree gets the same correspondences (exact nearest neighbours;
        // only the order of exactly equidistant points can differ) from a GridKNN built on the target once per tree.
        if (grid == nullptr && accelerate_kdtree_)
            if (const auto* kd = dynamic_cast<const knn::KDTree*>(&target_knn)) grid = grid_for(*kd, target);
        // every factor type searches on the grid when there is one (4x faster per k = 1 search than the KD-tree kernel);
        // GICP additionally fuses search and linearisation
        const knn::KNNBase& nn = (grid != nullptr && grid->size() == target.size()) ? static_cast<const knn::KNNBase&>(*grid)
                                                                                     : target_knn;
        // (the rotation constraint reads the raw covariances: it runs on the unfused kernels)
        const bool fused = grid != nullptr && grid->size() == target.size() && !params_.rotation_constraint.enable &&
                           (params_.reg_type == RegType::GICP || params_.reg_type == RegType::POINT_TO_DISTRIBUTION);
        fused_loop_active_ = fused;  // the LM / dog-leg trial steps then read the frozen correspondences from the cache
        if (fused) prepare_fused(source, target, *grid, initial_guess);
        // GICP + Gauss-Newton on a GridKNN: the whole loop runs on the device (one launch per iteration, convergence
        // test included), the host reads the result back once — same arithmetic as the loop below.
        // (the host-side pose terms — degenerate regularisation, MAP prior — need the reduced system on the host)
        const bool on_device = fused && !params_.verbose && params_.max_iterations > 0 && !pose_terms;
        const bool sharded = comm_ != nullptr || xchg_ != nullptr;
        // Every optimiser as ONE launch that loops on the device and ONE read-back (sp_gicp_align_optimize): LM and dog-leg always
        // (the reference crosses host <-> device 2 + inner tries times per iteration, registration.hpp:830-964), Gauss-Newton when
        // the source fits one workgroup (the pipeline's default 1000-point sample: no launch per iteration, no counter between
        // steps). std::nullopt: the launch is not available now, or its bounded wait ran out — the loops below take over.
        // A target with crowded cells — a raw scan: thousands of returns in the sensor's own cell — and a source of up to 131072
        // points: that launch with a WAVE per source point (sp_gicp_source_set_wave_per_point = 2), for Gauss-Newton too: a lane
        // alone walks thousands of candidates per query there (the reference's bundled scans at full resolution: 0.21 against
        // 0.69 ms per iteration). The fullest cell is measured once per grid (a kernel and a read-back, cached by the library).
        const bool crowded = on_device && !sharded && crowded_target(*grid, source.size());
        if (on_device && !sharded) throw_on_error(sp_gicp_source_set_wave_per_point(psrc_, crowded ? 2 : 1));
        if (on_device && !sharded &&
            (params_.optimization_method != OptimizationMethod::GAUSS_NEWTON || source.size() <= 1024 || crowded)) {
            const float scales[1] = {robust_scale};
            if (auto r = align_optimize_on_device(initial_guess, scales, 1)) return *r;
            prepare_fused(source, target, *grid, initial_guess);  // (the correspondence cache of the abandoned launch is stale)
        }
        if (on_device && params_.optimization_method == OptimizationMethod::GAUSS_NEWTON)
            return align_on_device(source.size(), initial_guess, robust_scale);
        if (comm_ != nullptr || xchg_ != nullptr)
            throw std::runtime_error("[Registration::align] a communicator is set: only the device-resident Gauss-Newton loop "
                                     "(GICP / POINT_TO_DISTRIBUTION on a GridKNN, no host-side pose terms) is sharded");

        return host_loop(initial_guess, robust_scale, pose_terms,
                         [&](const TransformMatrix& T) {
                             return fused ? linearize_fused(source.size(), T, robust_scale) : linearize_generic(source, target, nn, T, robust_scale);
                         },
                         [&](const TransformMatrix& T) { return compute_error(source, target, T, robust_scale); });
    }

    /// MI355X extension: align() with a photometric (intensity) term beside the geometric factor (Park, Zhou, Koltun,
    /// "Colored Point Cloud Registration Revisited", 2017). `target_gradients`: feature::compute_intensity_gradients_async of the
    /// target in its present frame; the source needs intensities. With params.photometric.weight > 0 the alignment runs the
    /// host-driven loop on the unfused kernels (the path the rotation constraint takes): every linearisation adds weight x the
    /// photometric system over the SAME correspondences before the pose terms, so the degenerate regulariser and the MAP prior see
    /// the combined system (H_raw / b_raw / error_raw are the combined system before them), and every trial error adds weight x the
    /// photometric error over the frozen correspondences. `inlier` stays the geometric count. With weight 0 this IS the overload
    /// without gradients. Not wired: RegistrationPipeline, the odometry pipelines, align_batch, align_global, the voxel-map overloads.
    RegistrationResult align(const PointCloudShared& source, const PointCloudShared& target, const knn::KNNBase& target_knn,
                             const feature::IntensityGradients& target_gradients,
                             const TransformMatrix& initial_guess = TransformMatrix::Identity(),
                             const ExecutionOptions& options = ExecutionOptions()) {
        const PhotometricParams& ph = params_.photometric;
        if (!(ph.weight > 0.0f)) return align(source, target, target_knn, initial_guess, options);
        // (nothing is enqueued before these)
        if (!source.has_intensity()) throw std::runtime_error("[Registration::align] the photometric term needs the intensities of the source");
        if (target_gradients.size() != target.size())
            throw std::invalid_argument("[Registration::align] target_gradients has another size than the target");
        if (comm_ != nullptr || xchg_ != nullptr)
            throw std::runtime_error("[Registration::align] a communicator is set: the photometric term runs on one device only");
        RegistrationResult result;
        result.T.matrix() = initial_guess;
        if (source.size() == 0) return result;
        validate_params(source, target, params_);
        const float robust_scale = options.robust_scale > 0.0f ? options.robust_scale : params_.robust.default_scale;
        rotation_robust_scale_ = options.rotation_robust_scale > 0.0f ? options.rotation_robust_scale
                                                                      : params_.rotation_constraint.robust.default_scale;
        const bool pose_terms = params_.degenerate_reg.type != DegenerateRegularizationType::none || prior_active();
        const auto* grid = dynamic_cast<const knn::GridKNN*>(&target_knn);
        if (grid == nullptr && accelerate_kdtree_)
            if (const auto* kd = dynamic_cast<const knn::KDTree*>(&target_knn)) grid = grid_for(*kd, target);
        const knn::KNNBase& nn = (grid != nullptr && grid->size() == target.size()) ? static_cast<const knn::KNNBase&>(*grid)
                                                                                     : target_knn;
        fused_loop_active_ = false;
        const sp_photometric_params pp{ph.weight, int(ph.robust_type), ph.robust_scale, params_.max_correspondence_distance};
        const float* const src_i = source.intensities->device_data();
        return host_loop(initial_guess, robust_scale, pose_terms,
                         [&](const TransformMatrix& T) {
                             LinearizedResult lin = linearize_generic(source, target, nn, T, robust_scale);
                             throw_on_error(sp_photometric_linearize(source.points_device(), src_i, source.size(), target.points_device(),
                                                                     target_gradients.device_data(), neighbors_.indices->device_data(),
                                                                     neighbors_.distances->device_data(), T.data(), 0, &pp, lin_dev_,
                                                                     nullptr, ws_, ws_bytes_, queue_.stream()));
                             const LinearizedResult photo = to_result(read_lin());
                             lin.H += photo.H * ph.weight;
                             lin.b += photo.b * ph.weight;
                             lin.error += ph.weight * photo.error;
                             return lin;
                         },
                         [&](const TransformMatrix& T) {
                             const auto [error, inlier] = compute_error(source, target, T, robust_scale);
                             throw_on_error(sp_photometric_error(source.points_device(), src_i, source.size(), target.points_device(),
                                                                 target_gradients.device_data(), neighbors_.indices->device_data(),
                                                                 neighbors_.distances->device_data(), T.data(), 0, &pp, lin_dev_, ws_,
                                                                 ws_bytes_, queue_.stream()));
                             return std::tuple<float, uint32_t>(error + ph.weight * read_lin().error, inlier);
                         });
    }

    /// MI355X extension: align() against the VoxelHashMap itself — voxelised GICP. The target of a source point is the Gaussian
    /// of the voxel T p falls into (set_voxel_neighbors(7) / (27): of the nearest voxel mean among that cell and its 6 face /
    /// all 26 neighbours); the correspondence is a hash lookup, so there is no export, no tree and no covariance estimation
    /// per keyframe (what Submap::build_submap pays to hand the other overload a target). GICP and POINT_TO_DISTRIBUTION, no
    /// rotation constraint. The map's registration rows are refreshed here when the map has changed since they were made.
    /// The optimiser loop is the host-driven one of the other overload: every OptimizationMethod, degenerate regularisation, the
    /// MAP prior, verbose.
    RegistrationResult align(const PointCloudShared& source, mapping::VoxelHashMap& target_map,
                             const TransformMatrix& initial_guess = TransformMatrix::Identity(),
                             const ExecutionOptions& options = ExecutionOptions()) {
        RegistrationResult result;
        result.T.matrix() = initial_guess;
        const size_t N = source.size();
        if (N == 0) return result;
        if ((params_.reg_type != RegType::GICP && params_.reg_type != RegType::POINT_TO_DISTRIBUTION) || params_.rotation_constraint.enable)
            throw std::invalid_argument("[Registration::align] a VoxelHashMap target: GICP or POINT_TO_DISTRIBUTION without the "
                                        "rotation constraint");
        if (params_.reg_type == RegType::GICP && !source.has_cov())
            throw std::runtime_error("[Registration::validate_params] Covariance matrices of source and target must be "
                                     "pre-computed before performing GICP matching.");
        if (comm_ != nullptr || xchg_ != nullptr)
            throw std::runtime_error("[Registration::align] a communicator is set: only the device-resident Gauss-Newton loop "
                                     "(GICP / POINT_TO_DISTRIBUTION on a GridKNN, no host-side pose terms) is sharded");
        if (params_.robust.type != robust::RobustLossType::NONE && params_.robust.default_scale <= 0.0f) {
            std::cout << "[Caution] `robust.default_scale` must be greater than zero. Disable robust loss." << std::endl;
            params_.robust.type = robust::RobustLossType::NONE;
        }
        const float robust_scale = options.robust_scale > 0.0f ? options.robust_scale : params_.robust.default_scale;
        const bool pose_terms = params_.degenerate_reg.type != DegenerateRegularizationType::none || prior_active();
        const int reg = int(params_.reg_type);
        if (!target_map.registration_ready(reg)) target_map.prepare_registration(reg);
        const size_t need = sp_vhm_registration_workspace_bytes(N);
        if (vws_bytes_ < need) {
            if (vws_) hip_check(hipFree(vws_), "hipFree");
            vws_ = nullptr; vws_bytes_ = 0;
            hip_check(hipMalloc(&vws_, need), "hipMalloc");
            vws_bytes_ = need;
        }
        throw_on_error(sp_vhm_prepare_source(source.covs_device(), N, reg, vws_, vws_bytes_, queue_.stream()));
        fused_loop_active_ = last_lin_fused_ = false;  // (compute_error_frozen: nothing of this alignment lies in neighbors_ or the cache)
        const sp_factor_params fp = factor_params(robust_scale);
        return host_loop(initial_guess, robust_scale, pose_terms,
                         [&](const TransformMatrix& T) {
                             throw_on_error(sp_vhm_linearize(target_map.handle(), source.points_device(), N, T.data(), 0, &fp, voxel_neighbors_,
                                                             lin_dev_, nullptr, vws_, vws_bytes_, queue_.stream()));
                             return to_result(read_lin());
                         },
                         [&](const TransformMatrix& T) {
                             throw_on_error(sp_vhm_error(target_map.handle(), source.points_device(), N, T.data(), 0, &fp, lin_dev_, vws_,
                                                         vws_bytes_, queue_.stream()));
                             const sp_linearized h = read_lin();
                             return std::tuple<float, uint32_t>{h.error, h.inlier};
                         });
    }
    /// The cells a source point probes in align(source, map): 1 (default) its own, 7 with the face neighbours, 27 all of 3x3x3.
    void set_voxel_neighbors(int neighbor_voxels) {
        if (neighbor_voxels != 1 && neighbor_voxels != 7 && neighbor_voxels != 27)
            throw std::invalid_argument("[Registration::set_voxel_neighbors] 1, 7 or 27");
        voxel_neighbors_ = neighbor_voxels;
    }
    int voxel_neighbors() const { return voxel_neighbors_; }

    /// MI355X extension: pipeline::RobustAligner's annealing loop (pipeline/robust.hpp:100-111) — one align() per robust scale,
    /// each starting from the pose the previous one ended on — with all levels in ONE launch and ONE read-back when align()
    /// would run on the device-resident optimiser (GICP / POINT_TO_DISTRIBUTION on a GridKNN or an accelerated KDTree, no
    /// rotation constraint, no host-side pose terms, not verbose); level by level through align() otherwise. Returns the last
    /// level's result, like the reference's loop.
    RegistrationResult align_levels(const PointCloudShared& source, const PointCloudShared& target, const knn::KNNBase& target_knn,
                                    const TransformMatrix& initial_guess, const ExecutionOptions& options,
                                    const std::vector<float>& robust_scales, const std::vector<float>& rotation_robust_scales) {
        RegistrationResult result;
        result.T.matrix() = initial_guess;
        if (source.size() == 0 || robust_scales.empty()) return result;
        const bool pose_terms = params_.degenerate_reg.type != DegenerateRegularizationType::none || prior_active();
        const bool candidate = robust_scales.size() > 1 && robust_scales.size() <= size_t(SP_OPT_MAX_LEVELS) && !params_.verbose &&
                               params_.max_iterations > 0 && !pose_terms && comm_ == nullptr && xchg_ == nullptr &&
                               !params_.rotation_constraint.enable &&
                               (params_.reg_type == RegType::GICP || params_.reg_type == RegType::POINT_TO_DISTRIBUTION);
        if (candidate) {
            validate_params(source, target, params_);
            const auto* grid = dynamic_cast<const knn::GridKNN*>(&target_knn);
            if (grid == nullptr && accelerate_kdtree_)
                if (const auto* kd = dynamic_cast<const knn::KDTree*>(&target_knn)) grid = grid_for(*kd, target);
            if (grid != nullptr && grid->size() == target.size() && params_.robust.type != robust::RobustLossType::NONE) {
                fused_loop_active_ = true;
                prepare_fused(source, target, *grid, initial_guess);
                const bool crowded = crowded_target(*grid, source.size());  // (see align())
                throw_on_error(sp_gicp_source_set_wave_per_point(psrc_, crowded ? 2 : 1));
                if (auto r = align_optimize_on_device(initial_guess, robust_scales.data(), (int)robust_scales.size())) return *r;
            }
        }
        for (size_t level = 0; level < robust_scales.size(); ++level) {  // pipeline/robust.hpp:100-111
            ExecutionOptions o = options;
            o.robust_scale = robust_scales[level];
            o.rotation_robust_scale = level < rotation_robust_scales.size() ? rotation_robust_scales[level] : options.rotation_robust_scale;
            result = align(source, target, target_knn, result.T.matrix(), o);
        }
        return result;
    }

    /// MI355X extension: align() from every pose of `initial_guesses` — relocalisation, start-up without a pose, a yaw sweep,
    /// loop-closure checks; the reference would call align() once per guess. With at least kAlignBatchMinGuesses guesses, a
    /// source of up to SP_ALIGN_BATCH_MAX_POINTS points and a configuration align() runs on its device-resident optimiser (GICP /
    /// POINT_TO_DISTRIBUTION on a GridKNN or an accelerated KDTree, no rotation constraint, no host-side pose terms, not verbose,
    /// max_iterations > 0, no communicator): ONE launch with a workgroup per guess (sp_gicp_align_batch), the poses up in one
    /// copy, the result blocks back in one read-back, the source prepared once, at initial_guesses[0]. Otherwise align() once
    /// per guess, so the call is always usable. result[i] belongs to initial_guesses[i]; best_of picks among them.
    /// A batch that ran on the device leaves NO frozen correspondences behind (each hypothesis kept its own, in scratch
    /// memory): compute_error_frozen throws after it, as it does before any alignment, until align() or
    /// compute_linearized_result() has run again — it never evaluates the rows of an earlier alignment by accident.
    std::vector<RegistrationResult> align_batch(const PointCloudShared& source, const PointCloudShared& target,
                                                const knn::KNNBase& target_knn, const std::vector<TransformMatrix>& initial_guesses,
                                                const ExecutionOptions& options = ExecutionOptions()) {
        std::vector<RegistrationResult> out;
        out.reserve(initial_guesses.size());
        const size_t B = initial_guesses.size(), N = source.size();
        const bool pose_terms = params_.degenerate_reg.type != DegenerateRegularizationType::none || prior_active();
        const knn::GridKNN* grid = nullptr;
        if (B >= kAlignBatchMinGuesses && B <= size_t(SP_ALIGN_BATCH_MAX) && N > 0 && N <= size_t(SP_ALIGN_BATCH_MAX_POINTS) &&
            !params_.verbose && params_.max_iterations > 0 && !pose_terms && comm_ == nullptr && xchg_ == nullptr &&
            !params_.rotation_constraint.enable &&
            (params_.reg_type == RegType::GICP || params_.reg_type == RegType::POINT_TO_DISTRIBUTION)) {
            validate_params(source, target, params_);
            grid = dynamic_cast<const knn::GridKNN*>(&target_knn);
            if (grid == nullptr && accelerate_kdtree_)
                if (const auto* kd = dynamic_cast<const knn::KDTree*>(&target_knn)) grid = grid_for(*kd, target);
            if (grid != nullptr && grid->size() != target.size()) grid = nullptr;
        }
        if (grid == nullptr) {
            for (const TransformMatrix& T0 : initial_guesses) out.push_back(align(source, target, target_knn, T0, options));
            return out;
        }
        const float robust_scale = options.robust_scale > 0.0f ? options.robust_scale : params_.robust.default_scale;
        prepare_fused(source, target, *grid, initial_guesses[0]);
        if (!sp_gicp_target_has_certificates(ptgt_)) {  // (the trial steps freeze on cache rows: only a certified target has them)
            throw_on_error(sp_gicp_target_certify(ptgt_, target.covs_device(), queue_.stream()));
            ptgt_covs_ = target.covs.get();
            ptgt_covs_gen_ = target.covs->generation();
        }
        const size_t rows_bytes = sp_gicp_align_batch_workspace_bytes(N, B);  // the hypotheses' cache rows
        return run_batch(initial_guesses, rows_bytes, [&](float* T_dev, sp_align_result* res_dev, char* workspace, size_t workspace_bytes) {
            const sp_factor_params fp = factor_params(robust_scale);
            const sp_opt_params op = opt_params();
            throw_on_error(sp_gicp_align_batch(ptgt_, psrc_, T_dev, T_dev, B, &fp, &op, &robust_scale, 1, res_dev, workspace,
                                               workspace_bytes, queue_.stream()));
        });
    }
    /// Where align_batch's one launch starts to win over align() per guess. Measured: a workgroup alone walks a
    /// 1000-point sample of a voxel-downsampled scan in 0.71 ms where the single launch, spread over the device, takes 0.2 ms, and
    /// every further guess adds about 0.02 ms to the batch: from 5 guesses on the batch is ahead (at 4: 0.95 of the sequential
    /// time); on a cloud of even density already from 2.
    static constexpr size_t kAlignBatchMinGuesses = 5;

    /// MI355X extension: align(source, map) from every pose of `initial_guesses` — relocalisation against the one target that
    /// persists across frames. With at least kVoxelAlignBatchMinGuesses guesses (and at most SP_ALIGN_BATCH_MAX), a source of up
    /// to SP_VHM_ALIGN_BATCH_MAX_POINTS points, not verbose, max_iterations in 1..65535, no degenerate regularisation, no active MAP
    /// prior: ONE optimiser launch with a workgroup per guess (sp_vhm_align_batch), the poses up in one copy, the result
    /// blocks back in one read-back. Otherwise align(source, map, guess) once per guess, so the call is always usable.
    /// Validation and messages are align(source, map)'s; voxel_neighbors() cells are probed; the map's registration rows are
    /// refreshed when they are stale. result[i] belongs to initial_guesses[i]; best_of picks among them. After a batch on the
    /// device nothing is frozen for compute_error_frozen, as after the other overload.
    std::vector<RegistrationResult> align_batch(const PointCloudShared& source, mapping::VoxelHashMap& target_map,
                                                const std::vector<TransformMatrix>& initial_guesses,
                                                const ExecutionOptions& options = ExecutionOptions()) {
        std::vector<RegistrationResult> out;
        out.reserve(initial_guesses.size());
        const size_t B = initial_guesses.size(), N = source.size();
        const bool pose_terms = params_.degenerate_reg.type != DegenerateRegularizationType::none || prior_active();
        if (!(B >= kVoxelAlignBatchMinGuesses && B <= size_t(SP_ALIGN_BATCH_MAX) && N > 0 && N <= size_t(SP_VHM_ALIGN_BATCH_MAX_POINTS) &&
              !params_.verbose && params_.max_iterations > 0 && params_.max_iterations <= 65535 && !pose_terms && comm_ == nullptr &&
              xchg_ == nullptr)) {  // (the launch logs the iteration in 16 bits: more iterations go guess by guess)
            for (const TransformMatrix& T0 : initial_guesses) out.push_back(align(source, target_map, T0, options));
            return out;
        }
        if ((params_.reg_type != RegType::GICP && params_.reg_type != RegType::POINT_TO_DISTRIBUTION) || params_.rotation_constraint.enable)
            throw std::invalid_argument("[Registration::align] a VoxelHashMap target: GICP or POINT_TO_DISTRIBUTION without the "
                                        "rotation constraint");
        if (params_.reg_type == RegType::GICP && !source.has_cov())
            throw std::runtime_error("[Registration::validate_params] Covariance matrices of source and target must be "
                                     "pre-computed before performing GICP matching.");
        if (params_.robust.type != robust::RobustLossType::NONE && params_.robust.default_scale <= 0.0f) {
            std::cout << "[Caution] `robust.default_scale` must be greater than zero. Disable robust loss." << std::endl;
            params_.robust.type = robust::RobustLossType::NONE;
        }
        const float robust_scale = options.robust_scale > 0.0f ? options.robust_scale : params_.robust.default_scale;
        const int reg = int(params_.reg_type);
        if (!target_map.registration_ready(reg)) target_map.prepare_registration(reg);
        const size_t ws_bytes = sp_vhm_align_batch_workspace_bytes(N, B);  // the source rows and the hypotheses' slots
        return run_batch(initial_guesses, ws_bytes, [&](float* T_dev, sp_align_result* res_dev, char* workspace, size_t workspace_bytes) {
            const sp_factor_params fp = factor_params(robust_scale);
            const sp_opt_params op = opt_params();
            throw_on_error(sp_vhm_align_batch(target_map.handle(), source.points_device(), source.has_cov() ? source.covs_device() : nullptr,
                                              N, T_dev, T_dev, B, &fp, &op, &robust_scale, 1, voxel_neighbors_, res_dev, nullptr, workspace,
                                              workspace_bytes, queue_.stream()));
        });
    }
    /// Where the voxel-map batch starts to win over align(source, map) per guess. Measured: already a single
    /// guess is ahead, 125 us against 341 us on 1000 points of the three planes and 319 us against 506 us on the bundled pair
    /// (one launch and one read-back against two launches and a read-back per step); at 256 guesses 31 and 43 times. Measured
    /// against the Python mirror's per-guess loop (its ctypes calls included) on sources of up to 6 124 points. A guess is one
    /// workgroup of 512 lanes: near SP_VHM_ALIGN_BATCH_MAX_POINTS a step is 32 passes on one compute unit, and one or two
    /// guesses of such a source have not been measured against the loop, which spreads a step over the device.
    static constexpr size_t kVoxelAlignBatchMinGuesses = 1;
    /// The best of align_batch's results by the rule of sp_align_best_host: the most inliers among results with a finite pose, a
    /// finite error and at least one inlier; ties to the smaller error, then to the lower index; results.size() when none qualifies.
    static size_t best_of(const std::vector<RegistrationResult>& results) {
        std::vector<sp_align_result> blocks(results.size());
        for (size_t i = 0; i < results.size(); ++i) {
            sp_align_result& h = blocks[i];
            h = sp_align_result{};
            std::memcpy(h.T, results[i].T.matrix().data(), sizeof h.T);
            h.error = results[i].error;
            h.inlier = results[i].inlier;
        }
        size_t best = results.size();
        throw_on_error(sp_align_best_host(blocks.data(), results.size(), &best));
        return best;
    }

    /// MI355X extension: align() without an initial guess (relocalisation when more than a yaw angle is unknown). The mutual
    /// nearest neighbours of the two clouds' FPFH rows (feature::compute_fpfh_async; consistently oriented normals) are the
    /// matches, params.hypotheses poses of matched triplets are scored by the matches they explain, the params.guesses best become
    /// the initial guesses of align_batch, and best_of picks the winner (global_registration.hpp: global_guesses). Fewer than three
    /// matches, no hypothesis that passes its gates, or no alignment best_of accepts: converged == false and the identity;
    /// nothing throws for want of matches. all_results / guesses_out receive every alignment and its initial guess.
    RegistrationResult align_global(const PointCloudShared& source, const feature::FPFHFeatures& source_features,
                                    const PointCloudShared& target, const feature::FPFHFeatures& target_features,
                                    const knn::KNNBase& target_knn, const GlobalRegistrationParams& global_params = GlobalRegistrationParams(),
                                    std::vector<RegistrationResult>* all_results = nullptr, std::vector<TransformMatrix>* guesses_out = nullptr,
                                    const ExecutionOptions& options = ExecutionOptions()) {
        return pick_global(global_guesses(source, source_features, target, target_features, global_params), all_results, guesses_out,
                           [&](const std::vector<TransformMatrix>& g) { return align_batch(source, target, target_knn, g, options); });
    }
    /// The same against a VoxelHashMap: `target` and its descriptors are the cloud the matches are drawn from (the scan or submap
    /// the map was built from), the alignment runs against the map (align_batch(source, map, guesses)).
    RegistrationResult align_global(const PointCloudShared& source, const feature::FPFHFeatures& source_features,
                                    const PointCloudShared& target, const feature::FPFHFeatures& target_features,
                                    mapping::VoxelHashMap& target_map, const GlobalRegistrationParams& global_params = GlobalRegistrationParams(),
                                    std::vector<RegistrationResult>* all_results = nullptr, std::vector<TransformMatrix>* guesses_out = nullptr,
                                    const ExecutionOptions& options = ExecutionOptions()) {
        return pick_global(global_guesses(source, source_features, target, target_features, global_params), all_results, guesses_out,
                           [&](const std::vector<TransformMatrix>& g) { return align_batch(source, target_map, g, options); });
    }

    /// MI355X extension: with a communicator set, `source` is THIS rank's shard of the source cloud (target, its
    /// covariances and its KNN structure are replicated on every rank) and align() runs the Gauss-Newton loop through
    /// sp_gicp_align_sharded: one launch and one 128-byte RCCL all-reduce per iteration, the identical pose on every rank.
    /// Applies where align() runs entirely on the device (GICP / POINT_TO_DISTRIBUTION on a GridKNN or an accelerated KDTree,
    /// Gauss-Newton, no host-side pose terms); every other configuration throws, since a rank-local result would silently
    /// differ between ranks. nullptr (default): single GPU.
    void set_communicator(sp_comm* comm) { comm_ = comm; }
    /// The same sharded alignment with the rows exchanged directly between the ranks' slot buffers (Exchange, sp_xchg):
    /// sp_gicp_align_direct, no collective launch per iteration. Takes precedence over a communicator. A peer that does
    /// not deliver within the exchange's timeout makes align() throw (SP_ERR_RUNTIME) on every waiting rank.
    void set_exchange(sp_xchg* xchg) { xchg_ = xchg; }

    /// MI355X extension: when align() is given a KDTree (no nodes removed) and the factor is GICP, search on a GridKNN
    /// built from the target instead (default on; results agree to rounding with the KD-tree path).
    void set_accelerate_kdtree(bool v) { accelerate_kdtree_ = v; }

    /// MI355X extension: tell align() that source clouds arrive spatially ordered (GridKNN::order() / voxel-downsampled
    /// clouds), so the prepared path skips its per-alignment sort (SP_SOURCE_PRESORTED).
    void set_source_presorted(bool v) { source_presorted_ = v; }

    /// registration.hpp:312-324: with the pose at the start of the optimisation window the degenerate regularisation
    /// is applied to the result.
    LinearizedResult compute_linearized_result(const PointCloudShared& source, const PointCloudShared& target,
                                               const knn::KNNBase& target_knn, const TransformMatrix& pose,
                                               const TransformMatrix& initial_pose,
                                               const ExecutionOptions& options = ExecutionOptions()) {
        LinearizedResult lin = compute_linearized_result(source, target, target_knn, pose, options);
        regularize(lin, pose, initial_pose);
        return lin;
    }
    /// registration.hpp:326-331 (without degenerate regularisation)
    LinearizedResult compute_linearized_result(const PointCloudShared& source, const PointCloudShared& target,
                                               const knn::KNNBase& target_knn, const TransformMatrix& pose,
                                               const ExecutionOptions& options = ExecutionOptions()) {
        const float s = options.robust_scale > 0.0f ? options.robust_scale : params_.robust.default_scale;
        rotation_robust_scale_ = options.rotation_robust_scale > 0.0f ? options.rotation_robust_scale
                                                                      : params_.rotation_constraint.robust.default_scale;
        return linearize_generic(source, target, target_knn, pose, s);
    }
    /// registration.hpp:350-359
    std::tuple<float, uint32_t> compute_error_frozen(const PointCloudShared& source, const PointCloudShared& target,
                                                     const TransformMatrix& pose,
                                                     const ExecutionOptions& options = ExecutionOptions()) const {
        const float s = options.robust_scale > 0.0f ? options.robust_scale : params_.robust.default_scale;
        rotation_robust_scale_ = options.rotation_robust_scale > 0.0f ? options.rotation_robust_scale
                                                                      : params_.rotation_constraint.robust.default_scale;
        // The reference evaluates the neighbours the last linearisation left in neighbors_ (registration.hpp:350-359). When
        // that linearisation ran on the prepared path (align() on a GridKNN / accelerated KDTree) they live in the
        // correspondence cache of the prepared source, frozen at lin_T_, not in neighbors_.
        fused_loop_active_ = last_lin_fused_;
        if (!last_lin_fused_ && (neighbors_.indices == nullptr || neighbors_.indices->size() != source.size()))
            throw std::runtime_error("[Registration::compute_error_frozen] no correspondences for this source: call align() or "
                                     "compute_linearized_result() first");
        return compute_error(source, target, pose, s);
    }
    /// registration.hpp:279-294
    void compute_icp_robust_weights(const PointCloudShared& source, const PointCloudShared& target,
                                    const knn::KNNBase& target_knn, const TransformMatrix& pose, float robust_scale,
                                    shared_vector<float>& out) const {
        const size_t N = source.size();
        out.assign(N, 0.0f);
        if (N == 0) return;
        target_knn.nearest_neighbor_search_async(source, neighbors_, {}, pose);
        last_lin_fused_ = false;
        const sp_factor_params fp = factor_params(robust_scale);
        throw_on_error(sp_icp_robust_weights(source.points_device(), source.covs_device(), N, target.points_device(),
                                             target.covs_device(), target.normals_device(), neighbors_.indices->device_data(),
                                             neighbors_.distances->device_data(), pose.data(), 0, &fp,
                                             out.device_data_for_write(N), queue_.stream()));
        queue_.wait();
    }
    const RegistrationParams& params() const { return params_; }
    /// MI355X extension: steps the latest device-resident optimiser run executed (linearisations, trial evaluations)
    std::pair<uint32_t, uint32_t> last_optimizer_steps() const { return {last_opt_linearizations_, last_opt_trials_}; }

private:
    /// The host-driven loop of align(): every decision of the optimiser (registration.hpp:803-964) is the library's stepper's — the
    /// state machine the device-resident launch runs (csrc/sp_optimizer.h); this loop linearises (linearize(T) -> LinearizedResult)
    /// and evaluates trials (trial_error(T) -> {error, inlier} over the correspondences of the last linearisation) where it asks.
    template <class Linearize, class TrialError>
    RegistrationResult host_loop(const TransformMatrix& initial_guess, float robust_scale, bool pose_terms, Linearize&& linearize,
                                 TrialError&& trial_error) {
        RegistrationResult result;
        const sp_opt_params op = opt_params();
        sp_opt_stepper* st = nullptr;
        throw_on_error(sp_opt_stepper_create(&op, initial_guess.data(), &robust_scale, 1, &st));
        const std::unique_ptr<sp_opt_stepper, void (*)(sp_opt_stepper*)> owner(st, sp_opt_stepper_destroy);
        for (;;) {
            sp_opt_request req;
            throw_on_error(sp_opt_stepper_next(st, &req));
            if (req.want == SP_OPT_WANT_DONE) break;
            TransformMatrix T;
            std::memcpy(T.data(), req.T, sizeof req.T);
            if (req.want == SP_OPT_WANT_LINEARIZE) {
                LinearizedResult lin = linearize(T);
                result.H_raw = lin.H; result.b_raw = lin.b; result.error_raw = lin.error;
                if (pose_terms) apply_pose_terms(lin, T, initial_guess);  // registration.hpp:249-253
                const sp_linearized h = to_linearized(lin);
                throw_on_error(sp_opt_stepper_linearized(st, &h));
                if (params_.verbose && params_.optimization_method == OptimizationMethod::GAUSS_NEWTON)
                    std::cout << "iter [" << req.iteration << "] error: " << lin.error << ", inlier: " << lin.inlier << std::endl;
            } else {
                const auto [icp_error, inlier] = trial_error(T);
                const float new_error = icp_error + prior_error(T);  // registration.hpp:854, :933
                float rho = 0.0f;
                throw_on_error(sp_opt_stepper_trial(st, new_error, inlier, &rho));
                if (params_.verbose && params_.optimization_method == OptimizationMethod::POWELL_DOGLEG)
                    std::cout << "iter [" << req.iteration << "] radius: " << req.damping << ", rho: " << rho
                              << ", error: " << new_error << ", inlier: " << inlier << std::endl;
            }
        }
        sp_align_result r;
        throw_on_error(sp_opt_stepper_result(st, &r));
        RegistrationResult out = to_registration_result(r);
        out.H_raw = result.H_raw; out.b_raw = result.b_raw; out.error_raw = result.error_raw;
        return out;
    }
    sp_factor_params factor_params(float robust_scale) const {
        return sp_factor_params{int(params_.reg_type), int(params_.robust.type), params_.max_correspondence_distance,
                                robust_scale, genz_alpha_, params_.genz.planarity_threshold,
                                params_.rotation_constraint.enable ? 1 : 0, params_.rotation_constraint.weight,
                                rotation_robust_scale_};
    }
    bool prior_active() const { return params_.map_prior.enabled && map_prior_.has_prior != 0; }
    float prior_error(const TransformMatrix& T) const {  // MapPrior::prior_error (map_prior.hpp:197-201)
        return prior_active() ? sp_map_prior_apply_host(&map_prior_, T.data(), nullptr, nullptr, nullptr) : 0.0f;
    }
    void regularize(LinearizedResult& lin, const TransformMatrix& T, const TransformMatrix& T_initial) const {
        if (params_.degenerate_reg.type == DegenerateRegularizationType::none) return;
        const sp_degenerate_reg_params dr{int(params_.degenerate_reg.type), params_.degenerate_reg.rot_eigenvalue_threshold,
                                          params_.degenerate_reg.trans_eigenvalue_threshold,
                                          params_.degenerate_reg.base_factor};
        sp_linearized h = to_linearized(lin);
        throw_on_error(sp_degenerate_regularize_host(&dr, h.H, h.b, h.inlier, T.data(), T_initial.data()));
        lin = to_result(h);
    }
    /// DegenerateRegularization::regularize then MapPrior::apply on the reduced system (registration.hpp:249-253)
    void apply_pose_terms(LinearizedResult& lin, const TransformMatrix& T, const TransformMatrix& T_initial) const {
        regularize(lin, T, T_initial);
        if (!prior_active()) return;
        sp_linearized h = to_linearized(lin);
        sp_map_prior_apply_host(&map_prior_, T.data(), h.H, h.b, &h.error);
        lin = to_result(h);
    }
    static LinearizedResult to_result(const sp_linearized& h) {
        LinearizedResult r;
        for (int i = 0; i < 6; ++i) {
            for (int j = 0; j < 6; ++j) r.H(i, j) = h.H[i * 6 + j];
            r.b(i) = h.b[i];
        }
        r.error = h.error;
        r.inlier = h.inlier;
        return r;
    }
    static sp_linearized to_linearized(const LinearizedResult& lin) {
        sp_linearized h{};
        for (int i = 0; i < 6; ++i) {
            for (int j = 0; j < 6; ++j) h.H[i * 6 + j] = lin.H(i, j);
            h.b[i] = lin.b(i);
        }
        h.error = lin.error;
        h.inlier = lin.inlier;
        return h;
    }
    /// sp_align_result (the device-resident optimiser's result block, the host stepper's read-out) as a RegistrationResult;
    /// H_raw / b_raw / error_raw as they are without host-side pose terms
    static RegistrationResult to_registration_result(const sp_align_result& h) {
        RegistrationResult result;
        for (int i = 0; i < 16; ++i) result.T.matrix().data()[i] = h.T[i];
        result.iterations = h.iterations;
        result.converged = h.converged != 0;
        for (int i = 0; i < 6; ++i) {
            for (int j = 0; j < 6; ++j) result.H(i, j) = h.H[i * 6 + j];
            result.b(i) = h.b[i];
        }
        result.error = h.error;
        result.inlier = h.inlier;
        result.H_raw = result.H; result.b_raw = result.b; result.error_raw = h.error_raw;
        return result;
    }
    /// The hand-off of both align_batch overloads: the poses up in one copy, `launch(T_dev, res_dev, workspace, workspace_bytes)`
    /// (the one C call, poses updated in place), the result blocks back in one read-back. Device: poses | result blocks |
    /// workspace; pinned host: poses | result blocks; both grown to the largest batch so far.
    template <class Launch>
    std::vector<RegistrationResult> run_batch(const std::vector<TransformMatrix>& guesses, size_t workspace_bytes, Launch&& launch) {
        const size_t B = guesses.size();
        const size_t poses_bytes = (B * 16 * sizeof(float) + 255) / 256 * 256, res_bytes = (B * sizeof(sp_align_result) + 255) / 256 * 256;
        if (batch_dev_bytes_ < poses_bytes + res_bytes + workspace_bytes) {
            if (batch_dev_) hip_check(hipFree(batch_dev_), "hipFree");
            batch_dev_ = nullptr; batch_dev_bytes_ = 0;
            hip_check(hipMalloc(&batch_dev_, poses_bytes + res_bytes + workspace_bytes), "hipMalloc");
            batch_dev_bytes_ = poses_bytes + res_bytes + workspace_bytes;
        }
        if (batch_pin_bytes_ < poses_bytes + res_bytes) {
            if (batch_pin_) hip_check(hipHostFree(batch_pin_), "hipHostFree");
            batch_pin_ = nullptr; batch_pin_bytes_ = 0;
            hip_check(hipHostMalloc(&batch_pin_, poses_bytes + res_bytes), "hipHostMalloc");
            batch_pin_bytes_ = poses_bytes + res_bytes;
        }
        float* const T_dev = reinterpret_cast<float*>(batch_dev_);
        sp_align_result* const res_dev = reinterpret_cast<sp_align_result*>(batch_dev_ + poses_bytes);
        float* const T_host = reinterpret_cast<float*>(batch_pin_);
        const sp_align_result* const res_host = reinterpret_cast<const sp_align_result*>(batch_pin_ + poses_bytes);
        for (size_t b = 0; b < B; ++b) std::memcpy(T_host + 16 * b, guesses[b].data(), 16 * sizeof(float));
        hip_check(hipMemcpyAsync(T_dev, T_host, B * 16 * sizeof(float), hipMemcpyHostToDevice, queue_.stream()), "H2D");
        launch(T_dev, res_dev, batch_dev_ + poses_bytes + res_bytes, workspace_bytes);
        hip_check(hipMemcpyAsync(batch_pin_ + poses_bytes, res_dev, B * sizeof(sp_align_result), hipMemcpyDeviceToHost, queue_.stream()), "D2H");
        hip_check(hipStreamSynchronize(queue_.stream()), "sync");
        std::vector<RegistrationResult> out;
        out.reserve(B);
        for (size_t b = 0; b < B; ++b) out.push_back(to_registration_result(res_host[b]));
        last_opt_linearizations_ = res_host[B - 1].linearizations;
        last_opt_trials_ = res_host[B - 1].trials;
        // nothing is frozen for compute_error_frozen: neither the source's cache nor neighbors_ describes this batch
        last_lin_fused_ = false;
        fused_loop_active_ = false;
        if (neighbors_.indices != nullptr) neighbors_.resize(0, 1);  // (never allocated when only maps have been aligned against)
        return out;
    }
    sp_linearized read_lin() const {  // the reference's wait_and_throw + toCPU(0) (registration.hpp:674-675)
        sp_linearized* const h = static_cast<sp_linearized*>(pin_);
        hip_check(hipMemcpyAsync(h, lin_dev_, sizeof *h, hipMemcpyDeviceToHost, queue_.stream()), "D2H");
        hip_check(hipStreamSynchronize(queue_.stream()), "sync");
        return *h;
    }
    float compute_genz_alpha(const PointCloudShared& target, size_t N) const {  // registration.hpp:464-511
        detail::DeviceScratch cnt(8);
        throw_on_error(sp_genz_counts(target.covs_device(), neighbors_.indices->device_data(),
                                      neighbors_.distances->device_data(), N, params_.max_correspondence_distance,
                                      params_.genz.planarity_threshold, static_cast<uint32_t*>(cnt.p), queue_.stream()));
        uint32_t h[2];
        hip_check(hipMemcpyAsync(h, cnt.p, 8, hipMemcpyDeviceToHost, queue_.stream()), "D2H");
        queue_.wait();
        return h[0] == 0 ? 1.0f : static_cast<float>(h[1]) / static_cast<float>(h[0]);
    }
    LinearizedResult linearize_generic(const PointCloudShared& source, const PointCloudShared& target,
                                       const knn::KNNBase& target_knn, const TransformMatrix& T, float robust_scale) {
        target_knn.nearest_neighbor_search_async(source, neighbors_, {}, T);
        last_lin_fused_ = false;
        if (params_.reg_type == RegType::GENZ) genz_alpha_ = compute_genz_alpha(target, source.size());
        const sp_factor_params fp = factor_params(robust_scale);
        throw_on_error(sp_gicp_linearize(source.points_device(), source.covs_device(), source.size(), target.points_device(),
                                         target.covs_device(), target.normals_device(), neighbors_.indices->device_data(),
                                         neighbors_.distances->device_data(), T.data(), 0, &fp, lin_dev_, ws_, ws_bytes_,
                                         queue_.stream()));
        return to_result(read_lin());
    }
    void prepare_fused(const PointCloudShared& source, const PointCloudShared& target, const knn::GridKNN& grid,
                       const TransformMatrix& T0) {
        // Reuse certificates (one k = 3 self-search of the target) pay when many source points are aligned to the target, or the
        // target is aligned to again (a submap, frame after frame). A target that is new and large beside its source — the
        // reference's example: a fresh 6 k-point target per frame, a 1000-point sample aligned to it — is prepared without them
        // (every linearisation then searches, seeded by the previous winner) and gets them if it comes back.
        const bool small_source = source.size() * 4 < target.size();
        if (ptgt_ == nullptr || ptgt_grid_id_ != grid.id()) {
            if (ptgt_) sp_gicp_target_destroy(ptgt_);
            ptgt_ = nullptr;
            if (small_source)
                throw_on_error(sp_gicp_target_create_plain(grid.handle(), target.covs_device(), target.size(), queue_.stream(), &ptgt_));
            else
                throw_on_error(sp_gicp_target_create(grid.handle(), target.covs_device(), target.size(), queue_.stream(), &ptgt_));
            ptgt_grid_id_ = grid.id();
            ptgt_covs_ = target.covs.get();  // (created with the GICP rows of these covariances)
            ptgt_covs_gen_ = target.covs->generation();
            ptgt_reg_ = int(RegType::GICP);
            ptgt_uses_ = 0;
        }
        ++ptgt_uses_;
        if ((ptgt_uses_ >= 2 || !small_source) && !sp_gicp_target_has_certificates(ptgt_)) {
            throw_on_error(sp_gicp_target_certify(ptgt_, target.covs_device(), queue_.stream()));
            ptgt_covs_ = target.covs.get();  // (the rows were rewritten from these covariances, for the factor they already served)
            ptgt_covs_gen_ = target.covs->generation();
        }
        // rows of the factor asked for: plane(Ct) for GICP, inverse(Ct) for point-to-distribution (factor.hpp:311-317) —
        // once per (target covariances, factor): a caller that aligns frame after frame against the same target does not pay
        // the 30 us per million points again (the container's generation moves whenever somebody may have written to it)
        if (ptgt_covs_ != target.covs.get() || ptgt_covs_gen_ != target.covs->generation() ||
            ptgt_reg_ != int(params_.reg_type)) {
            throw_on_error(sp_gicp_target_prepare(ptgt_, target.covs_device(), int(params_.reg_type), queue_.stream()));
            ptgt_covs_ = target.covs.get();
            ptgt_covs_gen_ = target.covs->generation();
            ptgt_reg_ = int(params_.reg_type);
        }
        if (psrc_ == nullptr || psrc_cap_ < source.size()) {
            if (psrc_) sp_gicp_source_destroy(psrc_);
            psrc_ = nullptr;
            throw_on_error(sp_gicp_source_create(source.size(), &psrc_));
            psrc_cap_ = source.size();
        }
        last_src_points_ = source.points_device();
        last_src_covs_ = source.covs_device();
        throw_on_error(sp_gicp_source_prepare(psrc_, ptgt_, last_src_points_, last_src_covs_, source.size(), T0.data(), 0,
                                              source_order(source.size()), queue_.stream()));
        neighbors_.indices == nullptr ? neighbors_.allocate(queue_, source.size(), 1) : neighbors_.resize(source.size(), 1);
    }
    /// How sp_gicp_source_prepare orders the source: as it is when the caller says it is spatially ordered — or when it is a few
    /// thousand points (the pipeline's random sample): the order only decides which lane handles which point, and the cell sort
    /// is seven launches for something a handful of waves do not notice.
    /// Whether a source of n points is better served by a wave per point against this target (measured: scratch/waveq_crossover.py,
    /// scratch/raw_scan_align.py, scratch/opt_example.py): a fullest cell of 512 points or more (a raw scan) for sources of up to
    /// 131072 points; of 32 or more (a voxel-downsampled scan: surfaces) up to 16384 — the reference example's whole 6 k-point
    /// source against its 6 k-point target: 0.28 against 0.37 ms per alignment. Up to 1024 points the launch takes that form by
    /// itself and the grid is not asked.
    static bool crowded_target(const knn::GridKNN& grid, size_t n) {
        if (n <= 1024 || n > 131072) return false;
        const uint32_t fullest = sp_grid_max_cell_points(grid.handle());
        return fullest >= 512 || (fullest >= 32 && n <= 16384);
    }
    int source_order(size_t n) const { return (source_presorted_ || n <= 4096) ? SP_SOURCE_PRESORTED : SP_SOURCE_SORT; }
    const knn::GridKNN* grid_for(const knn::KDTree& tree, const PointCloudShared& target) {
        if (!tree.pristine() || tree.size() != target.size() || target.size() == 0) return nullptr;
        if (kd_grid_ == nullptr || kd_grid_tree_id_ != tree.id()) {
            if (ptgt_) { sp_gicp_target_destroy(ptgt_); ptgt_ = nullptr; ptgt_grid_id_ = 0; }  // it borrows the old grid
            kd_grid_ = knn::GridKNN::build(queue_, target);
            kd_grid_tree_id_ = tree.id();
        }
        return kd_grid_.get();
    }
    sp_opt_params opt_params() const {
        return sp_opt_params{int(params_.optimization_method) == int(OptimizationMethod::GAUSS_NEWTON)          ? SP_OPT_GAUSS_NEWTON
                             : int(params_.optimization_method) == int(OptimizationMethod::LEVENBERG_MARQUARDT) ? SP_OPT_LEVENBERG_MARQUARDT
                                                                                                                 : SP_OPT_POWELL_DOGLEG,
                             (int)params_.max_iterations, params_.criteria.rotation, params_.criteria.translation, params_.gn.lambda,
                             (int)params_.lm.max_inner_iterations, params_.lm.lambda_factor, params_.lm.init_lambda,
                             params_.lm.max_lambda, params_.lm.min_lambda, params_.dogleg.initial_trust_region_radius,
                             params_.dogleg.min_trust_region_radius, params_.dogleg.max_trust_region_radius, params_.dogleg.eta1,
                             params_.dogleg.eta2, params_.dogleg.gamma_decrease, params_.dogleg.gamma_increase};
    }
    /// The prepared source / target are in place (prepare_fused): the whole optimiser loop — every level of `scales` — as one
    /// launch (sp_gicp_align_optimize) and one read-back. std::nullopt when the launch cannot be resident now or its bounded wait
    /// ran out (sp_align_result::status): the caller runs its per-step loop from the initial guess.
    std::optional<RegistrationResult> align_optimize_on_device(const TransformMatrix& initial_guess, const float* scales, int levels) {
        const sp_factor_params fp = factor_params(scales[0]);
        const sp_opt_params op = opt_params();
        sp_align_result* h;
        if (map_host_) {
            std::memcpy(map_host_, initial_guess.data(), 16 * sizeof(float));
            h = reinterpret_cast<sp_align_result*>(map_host_ + 256);
            volatile uint32_t* const done = &h->pad[0];
            *done = 0u;
            const int rc = sp_gicp_align_optimize(ptgt_, psrc_, reinterpret_cast<float*>(map_dev_), &fp, &op, scales, levels,
                                                  reinterpret_cast<sp_align_result*>(map_dev_ + 256), ws_, ws_bytes_, queue_.stream());
            if (rc == SP_ERR_RUNTIME && std::strstr(sp_last_error(), "not available") != nullptr) return std::nullopt;
            throw_on_error(rc);
            for (unsigned spins = 0; *done != SP_ALIGN_RESULT_DONE; ++spins) {
                if (spins > (1u << 24)) {  // (a fraction of a second: the device is busy elsewhere, or the launch failed — wait for the stream)
                    hip_check(hipStreamSynchronize(queue_.stream()), "sync");
                    break;
                }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
        } else {
            hip_check(hipMemcpyAsync(T_dev_, initial_guess.data(), 16 * sizeof(float), hipMemcpyHostToDevice, queue_.stream()), "H2D");
            const int rc = sp_gicp_align_optimize(ptgt_, psrc_, T_dev_, &fp, &op, scales, levels, res_dev_, ws_, ws_bytes_, queue_.stream());
            if (rc == SP_ERR_RUNTIME && std::strstr(sp_last_error(), "not available") != nullptr) return std::nullopt;
            throw_on_error(rc);
            h = reinterpret_cast<sp_align_result*>(static_cast<char*>(pin_) + 1024);
            hip_check(hipMemcpyAsync(h, res_dev_, sizeof *h, hipMemcpyDeviceToHost, queue_.stream()), "D2H");
            hip_check(hipStreamSynchronize(queue_.stream()), "sync");
        }
        if (h->status != 0) {  // not every workgroup of the launch was resident (another process / a CU mask holds compute units)
            throw_on_error(sp_gicp_source_set_persistent(psrc_, 0));  // this source: per-step launches from now on
            return std::nullopt;
        }
        for (int i = 0; i < 16; ++i) lin_T_.data()[i] = h->T_lin[i];
        last_lin_fused_ = true;
        last_opt_linearizations_ = h->linearizations;
        last_opt_trials_ = h->trials;
        return to_registration_result(*h);
    }
    RegistrationResult align_on_device(size_t N, const TransformMatrix& initial_guess, float robust_scale) {
        const sp_factor_params fp = factor_params(robust_scale);
        const sp_gn_params gn{params_.gn.lambda, params_.criteria.rotation, params_.criteria.translation};
        float* delta_dev = T_dev_ + 16;
        uint32_t* iters_dev = reinterpret_cast<uint32_t*>(T_dev_ + 24);
        hip_check(hipMemcpyAsync(T_dev_, initial_guess.data(), 16 * sizeof(float), hipMemcpyHostToDevice, queue_.stream()), "H2D");
        if (xchg_ != nullptr)  // source sharded over the ranks: rows stored into the peers' slot buffers
            throw_on_error(sp_gicp_align_direct(ptgt_, psrc_, T_dev_, &fp, &gn, (int)params_.max_iterations, xchg_, nullptr,
                                                nullptr, lin_dev_, delta_dev, iters_dev, ws_, ws_bytes_, queue_.stream()));
        else if (comm_ != nullptr)  // one 128-byte all-reduce per iteration
            throw_on_error(sp_gicp_align_sharded(ptgt_, psrc_, T_dev_, &fp, &gn, (int)params_.max_iterations, comm_, nullptr,
                                                 nullptr, lin_dev_, delta_dev, iters_dev, ws_, ws_bytes_, queue_.stream()));
        else
            // (no neighbour output: nothing reads neighbors_ on this path, and without it the kernels need not look for a
            // neighbour beyond max_correspondence_distance — with partial overlap that search was most of an iteration)
            throw_on_error(sp_gicp_align_fused(ptgt_, psrc_, T_dev_, &fp, &gn, (int)params_.max_iterations, nullptr, nullptr,
                                               lin_dev_, delta_dev, iters_dev, ws_, ws_bytes_, queue_.stream()));
        float* const host = reinterpret_cast<float*>(static_cast<char*>(pin_) + 256);  // pose | delta[8] | iterations | T_lin
        hip_check(hipMemcpyAsync(host, T_dev_, 28 * sizeof(float), hipMemcpyDeviceToHost, queue_.stream()), "D2H");
        // the pose the correspondence cache is frozen at (compute_error_frozen after align(), registration.hpp:350-359)
        throw_on_error(sp_gicp_align_linearization_pose(ws_, (int)params_.max_iterations - 1, host + 28, queue_.stream()));
        const sp_linearized h = read_lin();  // synchronises the stream
        if (xchg_ != nullptr)  // a row that did not arrive: the loop stopped, the pose is not the alignment's
            throw_on_error(sp_gicp_align_status(ws_, (int)params_.max_iterations - 1, queue_.stream()));
        const LinearizedResult lin = to_result(h);
        RegistrationResult result;
        TransformMatrix T;
        for (int i = 0; i < 16; ++i) T.data()[i] = host[i];
        for (int i = 0; i < 16; ++i) lin_T_.data()[i] = host[28 + i];
        last_lin_fused_ = true;
        result.T.matrix() = T;
        uint32_t iters;
        std::memcpy(&iters, &host[24], sizeof iters);
        if (iters == 0xffffffffu) {
            // the device-side tail of sp_gicp_align_fused ran into its bounded wait (not every workgroup was resident: another
            // process or a CU mask holds compute units) and left a NaN pose: once more from the initial guess, a launch per
            // iteration, and this prepared source stays on that form
            throw_on_error(sp_gicp_source_set_persistent(psrc_, 0));
            if (retried_without_persistent_)
                throw std::runtime_error("[Registration::align] the device-resident loop ran into its time limit");
            retried_without_persistent_ = true;
            throw_on_error(sp_gicp_source_prepare(psrc_, ptgt_, last_src_points_, last_src_covs_, N, initial_guess.data(), 0,
                                                  source_order(N), queue_.stream()));
            const RegistrationResult again = align_on_device(N, initial_guess, robust_scale);
            retried_without_persistent_ = false;
            return again;
        }
        result.iterations = iters > 0 ? iters - 1 : 0;  // index of the last iteration (registration.hpp:822)
        result.converged = host[16 + 6] > 0.5f;
        result.H = lin.H; result.b = lin.b; result.error = lin.error; result.inlier = lin.inlier;
        result.H_raw = lin.H; result.b_raw = lin.b; result.error_raw = lin.error;
        return result;
    }
    LinearizedResult linearize_fused(size_t N, const TransformMatrix& T, float robust_scale) {
        const sp_factor_params fp = factor_params(robust_scale);
        TransformMatrix Tc = T;
        lin_T_ = T;  // the pose the correspondences are frozen at (compute_error on the prepared path)
        last_lin_fused_ = true;
        throw_on_error(sp_gicp_iteration_fused(ptgt_, psrc_, Tc.data(), 0, &fp, nullptr, nullptr, nullptr, lin_dev_, nullptr, ws_,
                                               ws_bytes_, queue_.stream()));
        return to_result(read_lin());
    }
    std::tuple<float, uint32_t> compute_error(const PointCloudShared& source, const PointCloudShared& target,
                                              const TransformMatrix& T, float robust_scale) const {
        const sp_factor_params fp = factor_params(robust_scale);
        if (fused_loop_active_) {  // K12 over the correspondence cache: no gathers, no eigen-decompositions
            throw_on_error(sp_gicp_error_prepared(ptgt_, psrc_, lin_T_.data(), T.data(), 0, &fp, lin_dev_, ws_, ws_bytes_,
                                                  queue_.stream()));
            const sp_linearized h = read_lin();
            return {h.error, h.inlier};
        }
        throw_on_error(sp_gicp_error(source.points_device(), source.covs_device(), source.size(), target.points_device(),
                                     target.covs_device(), target.normals_device(), neighbors_.indices->device_data(),
                                     neighbors_.distances->device_data(), T.data(), 0, &fp, lin_dev_, ws_, ws_bytes_,
                                     queue_.stream()));
        const sp_linearized h = read_lin();
        return {h.error, h.inlier};
    }

    RegistrationParams params_;
    sycl_utils::DeviceQueue queue_;
    mutable knn::KNNResult neighbors_;
    sp_linearized* lin_dev_ = nullptr;
    void* ws_ = nullptr;
    size_t ws_bytes_ = 0;
    float* T_dev_ = nullptr;
    void* pin_ = nullptr;  // 4 KB of pinned host memory: [0, 256) linear system, [256, 432) pose | delta | iterations | T_lin,
                           // [1024, 1024 + sizeof(sp_align_result)) the result block of the device-resident optimiser
    sp_align_result* res_dev_ = nullptr;
    static constexpr size_t kMappedBytes = 256 + ((sizeof(sp_align_result) + 255) / 256) * 256;  // pose | result block
    char* map_host_ = nullptr;  // host-mapped: [0, 64) the optimiser's pose, [256, ...) its result block
    char* map_dev_ = nullptr;   // ... as the device sees it
    float genz_alpha_ = 1.0f;
    mutable float rotation_robust_scale_ = 10.0f;  // resolved per call from ExecutionOptions (registration.hpp:219-221)
    sp_map_prior_state map_prior_{};               // MapPrior state (map_prior.hpp:203-210)
    sp_gicp_source* psrc_ = nullptr;
    size_t psrc_cap_ = 0;
    sp_gicp_target* ptgt_ = nullptr;
    uint64_t ptgt_grid_id_ = 0;  // GridKNN::id() the prepared target was built on
    const void* ptgt_covs_ = nullptr;  // the covariance container the prepared rows were computed from, ...
    uint64_t ptgt_covs_gen_ = 0;       // ... its generation then, ...
    int ptgt_reg_ = -1;                // ... and the factor they are the rows of
    unsigned ptgt_uses_ = 0;           // alignments against this prepared target so far (second use: certificates, prepare_fused)
    bool source_presorted_ = false;
    sp_comm* comm_ = nullptr;  // borrowed (set_communicator)
    sp_xchg* xchg_ = nullptr;  // borrowed (set_exchange)
    bool accelerate_kdtree_ = true;
    mutable bool fused_loop_active_ = false;  // align() is running its optimiser loop on the prepared path
    mutable bool last_lin_fused_ = false;     // the last linearisation left its correspondences in the prepared source's cache
    TransformMatrix lin_T_ = TransformMatrix::Identity();  // pose of the last fused linearisation
    const float* last_src_points_ = nullptr;  // device pointers of the source of the latest prepare_fused (valid during align())
    const float* last_src_covs_ = nullptr;
    bool retried_without_persistent_ = false;
    uint32_t last_opt_linearizations_ = 0, last_opt_trials_ = 0;  // steps of the latest device-resident optimiser run
    template <class BatchFn>
    static RegistrationResult pick_global(std::vector<TransformMatrix> guesses, std::vector<RegistrationResult>* all_results,
                                          std::vector<TransformMatrix>* guesses_out, BatchFn&& batch) {
        std::vector<RegistrationResult> results;
        if (!guesses.empty()) results = batch(guesses);
        const size_t best = results.empty() ? 0 : best_of(results);
        RegistrationResult out = best < results.size() ? results[best] : RegistrationResult();
        if (all_results) *all_results = std::move(results);
        if (guesses_out) *guesses_out = std::move(guesses);
        return out;
    }
    char* batch_dev_ = nullptr;  // align_batch: poses | result blocks | per-hypothesis cache rows, grown to the largest batch so far
    size_t batch_dev_bytes_ = 0;
    char* batch_pin_ = nullptr;  // ... and pinned host memory for the poses going up and the blocks coming back
    size_t batch_pin_bytes_ = 0;
    void* vws_ = nullptr;  // align(source, map): partial rows | frozen slots | prepared source rows (sp_vhm_registration_workspace_bytes)
    size_t vws_bytes_ = 0;
    int voxel_neighbors_ = 1;
    knn::GridKNN::Ptr kd_grid_;        // GridKNN standing in for the caller's KDTree (grid_for)
    uint64_t kd_grid_tree_id_ = 0;
};

// ------------------------------------------------------------------------------------------------ pipeline wrappers
namespace pipeline {
/// pipeline/aligner.hpp:13-15
using RegistrationAligner = std::function<RegistrationResult(const PointCloudShared&, const PointCloudShared&,
                                                             const knn::KNNBase&, const TransformMatrix&,
                                                             const Registration::ExecutionOptions&)>;
inline RegistrationAligner make_registration_aligner(const Registration::Ptr& registration) {
    return [registration](const PointCloudShared& s, const PointCloudShared& t, const knn::KNNBase& k,
                          const TransformMatrix& T, const Registration::ExecutionOptions& o) {
        return registration->align(s, t, k, T, o);
    };
}
}  // namespace pipeline

/// registration_pipeline_params.hpp:11-43
struct RegistrationRandomSamplingParams {
    bool enable = true;
    size_t num = 1000;
    bool use_intensities = false;  // sample by the source's intensities (mixed_random_sampling) when it has them
    float weighted_ratio = 0.8f;   // the share of `num` drawn by weight on that path
};
struct RegistrationRobustScheduleParams {
    bool auto_scale = false;
    float init_scale = 10.0f, min_scale = 0.5f, rotation_init_scale = 10.0f, rotation_min_scale = 0.5f;
    size_t auto_scaling_iter = 4;
};
struct RegistrationVelocityUpdateParams { bool enable = false; size_t iter = 1; };
struct RegistrationPipelineParams {
    using RandomSampling = RegistrationRandomSamplingParams;
    using Robust = RegistrationRobustScheduleParams;
    using VelocityUpdate = RegistrationVelocityUpdateParams;
    RegistrationParams registration;
    RandomSampling random_sampling;
    Robust robust;
    VelocityUpdate velocity_update;
};

namespace pipeline {
/// pipeline/velocity_update.hpp:16-104 — repeats deskew and registration assuming constant sensor velocity: each round
/// deskews the source with the motion from options.prev_pose to the pose the previous round ended on (over options.dt), into
/// a cloud of its own, and aligns that.
class VelocityUpdateAligner {
public:
    using Ptr = std::shared_ptr<VelocityUpdateAligner>;
    VelocityUpdateAligner(RegistrationAligner aligner, size_t velocity_update_iter, bool verbose = false)
        : aligner_(std::move(aligner)), velocity_update_iter_(velocity_update_iter), verbose_(verbose) {}
    VelocityUpdateAligner(const Registration::Ptr& registration, size_t velocity_update_iter, bool verbose = false)
        : VelocityUpdateAligner(make_registration_aligner(registration), velocity_update_iter, verbose) {}
    RegistrationResult align(const PointCloudShared& source, const PointCloudShared& target, const knn::KNNBase& target_knn,
                             const TransformMatrix& initial_guess = TransformMatrix::Identity(),
                             const Registration::ExecutionOptions& options = Registration::ExecutionOptions()) const {
        RegistrationResult result;
        result.T.matrix() = initial_guess;
        if (source.size() == 0) return result;
        deskewed_pc_ = std::make_shared<PointCloudShared>(source.queue);  // the deskew writes into a cloud that aliases nothing
        if (!source.has_timestamps()) {
            if (verbose_) std::cout << "deskew skipped: source has no timestamps" << std::endl;
            *deskewed_pc_ = source;  // shallow
            return aligner_(*deskewed_pc_, target, target_knn, result.T.matrix(), options);
        }
        const Eigen::Isometry3f prev(options.prev_pose);
        const size_t rounds = std::max<size_t>(1, velocity_update_iter_);
        for (size_t round = 0; round < rounds; ++round) {
            if (verbose_) {
                float twist[6];
                sp_relative_twist_host(prev.matrix().data(), result.T.matrix().data(), twist);
                const float angle = std::sqrt(twist[0] * twist[0] + twist[1] * twist[1] + twist[2] * twist[2]);
                const float dist = std::sqrt(twist[3] * twist[3] + twist[4] * twist[4] + twist[5] * twist[5]);
                std::cout << "deskewed: " << round << std::endl;
                std::cout << "deskewed[" << round << "]: angle=" << angle << ", dist=" << dist << std::endl;
            }
            deskew::deskew_point_cloud_constant_velocity(source, *deskewed_pc_, prev, result.T, options.dt);
            result = aligner_(*deskewed_pc_, target, target_knn, result.T.matrix(), options);
        }
        return result;
    }
    /// the deskewed source of the most recent align(); null before the first
    const PointCloudShared::Ptr get_deskewed_point_cloud() const { return deskewed_pc_; }
    RegistrationAligner make_aligner() const {
        return [this](const PointCloudShared& s, const PointCloudShared& t, const knn::KNNBase& k, const TransformMatrix& T,
                      const Registration::ExecutionOptions& o) { return this->align(s, t, k, T, o); };
    }

private:
    RegistrationAligner aligner_;
    size_t velocity_update_iter_ = 1;
    bool verbose_ = false;
    mutable PointCloudShared::Ptr deskewed_pc_ = nullptr;
};

/// pipeline/robust.hpp:17-128 — geometric annealing of the robust scale around the wrapped aligner.
class RobustAligner {
public:
    using Ptr = std::shared_ptr<RobustAligner>;
    RobustAligner(RegistrationAligner aligner, const RegistrationPipelineParams& p)
        : aligner_(std::move(aligner)), params_(p.registration), sched_(p.robust) {}
    /// pipeline/robust.hpp:32-33. With the backend known, the levels go to Registration::align_levels: one launch, one
    /// read-back for the whole schedule where the device-resident optimiser applies, the same loop as below otherwise.
    RobustAligner(const Registration::Ptr& registration, const RegistrationPipelineParams& p)
        : RobustAligner(make_registration_aligner(registration), p) {
        registration_ = registration;
    }
    RegistrationResult align(const PointCloudShared& source, const PointCloudShared& target, const knn::KNNBase& knn,
                             const TransformMatrix& initial_guess = TransformMatrix::Identity(),
                             const Registration::ExecutionOptions& options = Registration::ExecutionOptions()) const {
        RegistrationResult result;
        result.T.matrix() = initial_guess;
        if (source.size() == 0) return result;
        const bool fixed = options.robust_scale > 0.0f || options.rotation_robust_scale > 0.0f;
        bool autos = !fixed && params_.robust.type != robust::RobustLossType::NONE && sched_.auto_scale;
        if (autos && (sched_.min_scale <= 0.0f || sched_.min_scale >= sched_.init_scale)) autos = false;
        if (autos && (sched_.rotation_min_scale <= 0.0f || sched_.rotation_min_scale >= sched_.rotation_init_scale)) autos = false;
        if (autos && sched_.auto_scaling_iter == 0) autos = false;
        const size_t levels = autos ? std::max<size_t>(1, sched_.auto_scaling_iter) : 1;
        // pipeline/robust.hpp:83-98: both scales shrink geometrically from init to min over the levels
        float scale = options.robust_scale > 0.0f ? options.robust_scale
                                                  : (autos ? sched_.init_scale : params_.robust.default_scale);
        const float factor = levels > 1 ? std::pow(sched_.min_scale / sched_.init_scale, 1.0f / static_cast<float>(levels - 1)) : 1.0f;
        float rot_scale = options.rotation_robust_scale > 0.0f
                              ? options.rotation_robust_scale
                              : (autos ? sched_.rotation_init_scale : params_.rotation_constraint.robust.default_scale);
        const float rot_factor =
            levels > 1 ? std::pow(sched_.rotation_min_scale / sched_.rotation_init_scale, 1.0f / static_cast<float>(levels - 1)) : 1.0f;
        if (registration_ != nullptr) {
            std::vector<float> scales, rot_scales;
            for (size_t level = 0; level < levels; ++level) {
                scales.push_back(scale);
                rot_scales.push_back(rot_scale);
                scale *= factor;
                rot_scale *= rot_factor;
            }
            return registration_->align_levels(source, target, knn, initial_guess, options, scales, rot_scales);
        }
        for (size_t level = 0; level < levels; ++level) {
            auto o = options;
            o.robust_scale = scale;
            o.rotation_robust_scale = rot_scale;
            result = aligner_(source, target, knn, result.T.matrix(), o);
            scale *= factor;
            rot_scale *= rot_factor;
        }
        return result;
    }
    RegistrationAligner make_aligner() const {
        return [this](const PointCloudShared& s, const PointCloudShared& t, const knn::KNNBase& k, const TransformMatrix& T,
                      const Registration::ExecutionOptions& o) { return this->align(s, t, k, T, o); };
    }

private:
    RegistrationAligner aligner_;
    RegistrationParams params_;
    RegistrationRobustScheduleParams sched_;
    Registration::Ptr registration_;  // set when the wrapped aligner IS a Registration backend
};
}  // namespace pipeline

/// registration_pipeline.hpp:16-149 — optional random sampling of the source, then (annealed) alignment, each level through the
/// optional deskew-and-realign rounds of the velocity update.
class RegistrationPipeline {
public:
    using Ptr = std::shared_ptr<RegistrationPipeline>;
    /// registration_pipeline.hpp:24-43: from an aligner callable, from a Registration backend, or from a queue
    RegistrationPipeline(pipeline::RegistrationAligner aligner, const RegistrationPipelineParams& p = RegistrationPipelineParams())
        : params_(p), aligner_(std::move(aligner)) {
        wrap_aligner();
    }
    RegistrationPipeline(const Registration::Ptr& registration, const RegistrationPipelineParams& p = RegistrationPipelineParams())
        : params_(p), registration_(registration), aligner_(pipeline::make_registration_aligner(registration)) {
        wrap_aligner();
    }
    RegistrationPipeline(const sycl_utils::DeviceQueue& queue, const RegistrationPipelineParams& p = RegistrationPipelineParams())
        : RegistrationPipeline(std::make_shared<Registration>(queue, p.registration), p) {}

    RegistrationResult align(const PointCloudShared& source, const PointCloudShared& target, const knn::KNNBase& target_knn,
                             const TransformMatrix& initial_guess = TransformMatrix::Identity(),
                             const Registration::ExecutionOptions& options = Registration::ExecutionOptions()) const {
        update_registration_input(source);
        return aligner_(*input_, target, target_knn, initial_guess, options);
    }
    const Registration::Ptr& registration() const { return registration_; }
    /// registration_pipeline.hpp:64-77: geometry ICP robust weights of the latest registration input
    void compute_icp_robust_weights(const PointCloudShared& target, const knn::KNNBase& target_knn, const TransformMatrix& pose,
                                    float robust_scale, shared_vector<float>& out) const {
        if (registration_ == nullptr)
            throw std::runtime_error("[RegistrationPipeline::compute_icp_robust_weights] Registration backend is not available.");
        const auto source = get_deskewed_point_cloud();
        if (source == nullptr)
            throw std::runtime_error("[RegistrationPipeline::compute_icp_robust_weights] Registration input point cloud is not available.");
        registration_->compute_icp_robust_weights(*source, target, target_knn, pose, robust_scale, out);
    }
    const PointCloudShared* get_registration_input_point_cloud() const { return input_.get(); }
    /// registration_pipeline.hpp:82-89: the deskewed source of the latest align(); the registration input with velocity_update off
    const PointCloudShared::Ptr get_deskewed_point_cloud() const {
        if (velocity_update_ != nullptr) return velocity_update_->get_deskewed_point_cloud();
        return input_;
    }
    /// registration_pipeline.hpp:91-97
    float get_inlier_ratio(const RegistrationResult& result) const {
        const auto* in = get_registration_input_point_cloud();
        if (in && in->size() > 0) return static_cast<float>(result.inlier) / static_cast<float>(in->size());
        return 0.0f;
    }

private:
    /// registration_pipeline.hpp:100-119: RobustAligner -> VelocityUpdateAligner -> base aligner (for each robust scale, for each
    /// deskew update: align)
    void wrap_aligner() {
        if (params_.velocity_update.enable) {
            velocity_update_ = std::make_shared<pipeline::VelocityUpdateAligner>(aligner_, params_.velocity_update.iter,
                                                                                 params_.registration.verbose);
            aligner_ = velocity_update_->make_aligner();
        }
        if (params_.robust.auto_scale) {
            // (with nothing between the two the robust wrapper talks to the backend: all levels in one launch; with the velocity
            // update in between it is the host loop over the levels, each inner Registration::align one device-resident launch)
            robust_ = registration_ != nullptr && velocity_update_ == nullptr
                          ? std::make_shared<pipeline::RobustAligner>(registration_, params_)
                          : std::make_shared<pipeline::RobustAligner>(aligner_, params_);
            aligner_ = robust_->make_aligner();
        }
    }
    void update_registration_input(const PointCloudShared& source) const {  // registration_pipeline.hpp:121-140
        if (filter_ == nullptr || input_ == nullptr) {
            filter_ = std::make_shared<filter::PreprocessFilter>(source.queue);
            input_ = std::make_shared<PointCloudShared>(source.queue);
        }
        const auto& rs = params_.random_sampling;
        if (rs.enable && source.size() > rs.num) {
            if (rs.use_intensities && source.has_intensity())
                filter_->mixed_random_sampling(source, *input_, *source.intensities, rs.num, rs.weighted_ratio);
            else filter_->random_sampling(source, *input_, rs.num);
        } else *input_ = source;  // shallow (registration_pipeline.hpp:138)
    }
    RegistrationPipelineParams params_;
    Registration::Ptr registration_;
    pipeline::RobustAligner::Ptr robust_;
    pipeline::VelocityUpdateAligner::Ptr velocity_update_;
    pipeline::RegistrationAligner aligner_;
    mutable filter::PreprocessFilter::Ptr filter_;
    mutable PointCloudShared::Ptr input_;
};

}  // namespace registration
}  // namespace algorithms
}  // namespace sycl_points
