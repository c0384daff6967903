// sycl_points facade for MI355X — covariance / normals, voxel grid, pre-filters, transform.
//   algorithms/feature/covariance.hpp            : covariance::estimate_async, estimate_normals_async, extract_normals(_async)
//   algorithms/filter/voxel_downsampling.hpp     : filter::VoxelGrid
//   algorithms/filter/polar_downsampling.hpp     : filter::PolarGrid
//   algorithms/common/coordinate_system.hpp      : CoordinateSystem, coordinate_system_from_string
//   algorithms/filter/preprocess_filter.hpp      : filter::PreprocessFilter (box_filter, random_sampling, weighted_random_sampling,
//                                                  mixed_random_sampling, farthest_point_sampling, angle_incidence_filter)
//   algorithms/filter/intensity_correction.hpp   : intensity_correction::correct_intensity
//   algorithms/filter/intensity_gaussian.hpp     : intensity_gaussian::smooth_intensity
//   algorithms/filter/intensity_local_mean_norm.hpp : intensity_local_mean_norm::normalize
//   algorithms/filter/intensity_zscore.hpp       : intensity_zscore::compute
//   algorithms/filter/outlier_removal_filter.hpp : filter::OutlierRemoval (statistical, radius)
//   algorithms/common/filter_by_flags.hpp        : filter::FilterByFlags
//   algorithms/common/transform.hpp              : transform::transform, transform_copy
//   (no header of the reference)                 : feature::FPFHFeatures, feature::compute_fpfh(_async) — MI355X extension
//   (no header of the reference)                 : feature::IntensityGradients, feature::compute_intensity_gradients(_async) — MI355X extension
#pragma once
#include <exception>
#include <mutex>
#include <utility>
#include <vector>
#include <cctype>
#include <cmath>
#include <iostream>
#include <limits>
#include <numeric>
#include <random>
#include <stdexcept>
#include <unordered_map>

#include "knn.hpp"

namespace sycl_points {
namespace algorithms {

namespace detail {
/// Scratch device memory that lives for one call (the reference allocates shared_vectors per call the same way,
/// e.g. registration.hpp:685-686).
// Device scratch of one call (workspaces, counters), from the cache the containers use (core.hpp: keyed by device, no
// hipMalloc / hipFree per call). Every user synchronises its stream before the scratch leaves scope, so the buffer goes
// back idle; when the scope is left by an exception that may not have happened yet, and the device is drained first.
struct DeviceScratch {
    void* p = nullptr;
    size_t bytes = 0;
    /// st: the stream the scratch will be used on (a buffer last used on the same stream is taken without waiting)
    explicit DeviceScratch(size_t n, hipStream_t st = nullptr) : st_(st) {
        if (n) p = ::sycl_points::detail::DeviceBufferCache::acquire(n, &bytes, st);
    }
    ~DeviceScratch() {
        if (!p) return;
        if (std::uncaught_exceptions() > 0) (void)hipDeviceSynchronize();
        if (stream_ordered) ::sycl_points::detail::DeviceBufferCache::release(p, bytes, st_, /*idle=*/false);
        else ::sycl_points::detail::DeviceBufferCache::release(p, bytes, nullptr, /*idle=*/true);
    }
    /// set by a user that did NOT synchronise: everything that touched the scratch was enqueued on the stream it was taken for
    bool stream_ordered = false;
    hipStream_t st_ = nullptr;
    DeviceScratch(const DeviceScratch&) = delete;
    DeviceScratch& operator=(const DeviceScratch&) = delete;
};
// One 4-byte read-back through pinned memory (a copy into pageable memory is staged and blocks inside the runtime).
inline void* pinned_word() {
    static void* p = [] { void* q = nullptr; hip_check(hipHostMalloc(&q, 64), "hipHostMalloc"); return q; }();
    return p;
}
/// 4 KB of pinned host memory per host thread for read-backs of a few hundred bytes (nullptr: none to be had)
inline void* pinned_block_4k() {
    thread_local void* p = [] {
        void* q = nullptr;
        if (hipHostMalloc(&q, 4096, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); q = nullptr; }
        return q;
    }();
    return p;
}
/// A count a kernel hands to the host WITHOUT a copy and a stream synchronisation: the kernel stores it through the device
/// pointer of a host-mapped pinned word, the host spins on the word (armed with a value no count takes). A D2H copy + a
/// hipStreamSynchronize is 15-20 us of runtime calls and wake-up for four bytes; the spin sees the store a microsecond or two
/// after it lands. Later work on the stream stays ordered behind the kernel as ever; the kernel's OTHER outputs may still be in
/// flight when the count arrives (they stay on the device). One word per host thread.
struct MappedWord {
    volatile uint32_t* host = nullptr;
    uint32_t* dev = nullptr;
    static constexpr uint32_t kArmed = 0xffffffffu;
    static MappedWord& mine() {
        thread_local MappedWord w = [] {
            MappedWord m;
            void* h = nullptr;
            if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return m; }  // (every device of the process may store to it)
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(h); return m; }
            m.host = static_cast<volatile uint32_t*>(h);
            m.dev = static_cast<uint32_t*>(d);
            return m;
        }();
        return w;
    }
    bool usable() const { return host != nullptr; }
    void arm() const { *host = kArmed; }
    /// the value once the kernel has stored it; a stream error (the kernel never ran) ends the wait through the synchronisation
    uint32_t wait(hipStream_t st) const {
        for (unsigned spins = 0;; ++spins) {
            const uint32_t v = *host;
            if (v != kArmed) return v;
            if (spins > (1u << 22)) {  // (tens of milliseconds: something is wrong or the device is very busy — fall back to waiting)
                hip_check(hipStreamSynchronize(st), "sync");
                return *host;
            }
        }
    }
};
inline uint32_t read_u32(const void* dev, hipStream_t st) {
    static std::mutex m;  // one pinned word for the process: read-backs are short and rare
    std::lock_guard<std::mutex> lock(m);
    uint32_t* const v = static_cast<uint32_t*>(pinned_word());
    hip_check(hipMemcpyAsync(v, dev, 4, hipMemcpyDeviceToHost, st), "D2H");
    hip_check(hipStreamSynchronize(st), "sync");
    return *v;
}
/// The protocol of VoxelGrid::run and PolarGrid::run around one sp_voxel_downsample_report / sp_polar_downsample_report call
/// (run(): key_box(box6_dev) computes a cloud's key box on the device, report(box6_host, report8, workspace, workspace_bytes)
/// enqueues the call). Returns the call's record {voxels, points outside the box, this cloud's key box lo xyz, hi xyz}.
class KeyBoxMemory {
public:
    void forget() { have_key_box_ = false; }
    template <class KeyBoxFn, class ReportFn>
    std::array<int32_t, 8> run(size_t N, hipStream_t st, KeyBoxFn&& key_box, ReportFn&& report) {
        const size_t ws_bytes = sp_voxel_downsample_workspace_bytes(N);
        // voxel count | boxed-path status | key box of the key-box call (6 ints) | this cloud's key box, sharded
        constexpr int kInfoInts = 32 + SP_VOXEL_BOX_SHARD_STRIDE * SP_VOXEL_BOX_SHARDS;
        DeviceScratch ws(ws_bytes, st), info(kInfoInts * 4, st);
        uint32_t* info_dev = static_cast<uint32_t*>(info.p);
        static_assert(kInfoInts * 4 <= 4096, "pinned block");
        int32_t h_own[kInfoInts];
        int32_t* const h = pinned_block_4k() ? static_cast<int32_t*>(pinned_block_4k()) : h_own;  // (read-backs by DMA)
        // The sort runs on keys compressed to the (widened) key box of the PREVIOUS cloud — scans of one sensor have similar
        // extents; the device verifies that this cloud fits, and the key kernel finds this cloud's own box on the way (next
        // call's guess; the exact box of the redo when the cloud did not fit). The first call has no guess and computes the
        // box first: every call sorts compressed keys (the 64-bit sort is left for boxes of >= 2^32 cells).
        // The call reports {voxels, points outside the box, this cloud's key box} in ONE record (sp_voxel_downsample_report): through
        // host-mapped words the last kernel stores to and this thread spins on when they are to be had — no copy, no
        // synchronisation: the scratch then goes back behind the stream's work — else through a copy and a wait.
        const MappedWord& mapped = MappedWord::mine();
        const bool poll = mapped.usable();
        auto launch = [&](const int32_t* box) {
            uint32_t* const rep = poll ? mapped.dev : info_dev;
            if (poll) mapped.arm();
            report(box, rep, ws.p, ws_bytes);
            if (poll) {
                h[0] = static_cast<int32_t>(mapped.wait(st));
                std::atomic_thread_fence(std::memory_order_acquire);
                for (int j = 1; j < 8; ++j) h[j] = static_cast<int32_t>(mapped.host[j]);
                ws.stream_ordered = true;  // (kernels of the call may still be running: not idle, but ordered on st)
                info.stream_ordered = true;
            } else {
                hip_check(hipMemcpyAsync(h, info.p, 32, hipMemcpyDeviceToHost, st), "D2H");
                hip_check(hipStreamSynchronize(st), "sync");
            }
        };
        if (!have_key_box_) {
            key_box(reinterpret_cast<int32_t*>(info_dev + 2));
            hip_check(hipMemcpyAsync(h, info.p, 32, hipMemcpyDeviceToHost, st), "D2H");
            hip_check(hipStreamSynchronize(st), "sync");
            have_key_box_ = h[2] <= h[5] && h[3] <= h[6] && h[4] <= h[7];
            for (int a = 0; a < 6; ++a) key_box_[a] = h[2 + a];
        }
        launch(have_key_box_ ? key_box_ : nullptr);
        if (h[1] != 0) {  // the cloud left the remembered box: again, with its own
            int32_t exact[6] = {h[2], h[3], h[4], h[5], h[6], h[7]};
            launch(exact);
        }
        const bool had_box = have_key_box_;
        have_key_box_ = h[2] <= h[5] && h[3] <= h[6] && h[4] <= h[7];
        if (have_key_box_) {
            // Keep what earlier clouds needed as well (one VoxelGrid usually serves several scans in turn — source and target of
            // a registration —, and a guess that forgets the other scan is redone every call), unless that has grown to more
            // than 8x the cells this cloud needs.
            int32_t lo[3], hi[3], ulo[3], uhi[3];
            double cells = 1.0, ucells = 1.0;
            for (int a = 0; a < 3; ++a) {
                const int32_t margin = std::max<int32_t>(2, (h[5 + a] - h[2 + a] + 1) / 8);
                lo[a] = std::max<int32_t>(h[2 + a] - margin, 0);
                hi[a] = std::min<int32_t>(h[5 + a] + margin, (1 << 21) - 1);
                ulo[a] = had_box ? std::min(lo[a], key_box_[a]) : lo[a];
                uhi[a] = had_box ? std::max(hi[a], key_box_[3 + a]) : hi[a];
                cells *= double(hi[a] - lo[a] + 1);
                ucells *= double(uhi[a] - ulo[a] + 1);
            }
            const bool keep = ucells <= 8.0 * cells;
            for (int a = 0; a < 3; ++a) {
                key_box_[a] = keep ? ulo[a] : lo[a];
                key_box_[3 + a] = keep ? uhi[a] : hi[a];
            }
        }
        std::array<int32_t, 8> rec;
        for (int j = 0; j < 8; ++j) rec[j] = h[j];
        return rec;
    }

private:
    int32_t key_box_[6] = {0, 0, 0, 0, 0, 0};
    bool have_key_box_ = false;
};
/// What VoxelGrid::run and PolarGrid::run share: KeyBoxMemory's protocol around the class's two C calls. key_box(box6_dev) is its
/// sp_*_key_box; downsample(tail...) its sp_*_downsample_report, handed the arguments both end with, from `rgb` on: the inputs the
/// cloud has, the outputs sized for N rows at every launch. The outputs then get the V voxels the record (returned) reports.
template <class KeyBoxFn, class DownsampleFn>
std::array<int32_t, 8> downsample_run(KeyBoxMemory& boxes, hipStream_t st, size_t N, const RGBContainerShared* rgb,
                                      const IntensityContainerShared* inten, const TimestampContainerShared* ts,
                                      PointContainerShared& out_pts, RGBContainerShared* out_rgb, IntensityContainerShared* out_inten,
                                      TimestampContainerShared* out_ts, KeyBoxFn&& key_box, DownsampleFn&& downsample) {
    const std::array<int32_t, 8> h = boxes.run(N, st, key_box, [&](const int32_t* box, uint32_t* report, void* ws, size_t ws_bytes) {
        downsample(rgb ? reinterpret_cast<const float*>(rgb->device_data()) : nullptr, inten ? inten->device_data() : nullptr,
                   ts ? ts->device_data() : nullptr, reinterpret_cast<float*>(out_pts.device_data_for_write(N)),
                   rgb ? reinterpret_cast<float*>(out_rgb->device_data_for_write(N)) : nullptr,
                   inten ? out_inten->device_data_for_write(N) : nullptr, ts ? out_ts->device_data_for_write(N) : nullptr,
                   static_cast<uint64_t*>(nullptr), static_cast<uint32_t*>(nullptr), box, report, ws, ws_bytes, st);
    });
    const size_t V = static_cast<uint32_t>(h[0]);
    out_pts.set_device_size(V);
    if (rgb) out_rgb->set_device_size(V);
    if (inten) out_inten->set_device_size(V);
    if (ts) out_ts->set_device_size(V);
    return h;
}
/// VoxelGrid's and PolarGrid's downsampling(cloud, result) around the class's run(points, N, the three inputs the cloud has, the
/// four outputs): in place allowed; the result has no covariances and normals, and the cloud's times when it has timestamps.
template <class RunFn>
void downsample_cloud(const sycl_utils::DeviceQueue& queue, const PointCloudShared& cloud, PointCloudShared& result, RunFn&& run) {
    const size_t N = cloud.size();
    if (N == 0) { result.resize_points(0); return; }
    const bool in_place = (&cloud == &result) || (cloud.points == result.points);
    PointCloudShared tmp(queue);
    PointCloudShared& out = in_place ? tmp : result;
    run(cloud.points_device(), N, cloud.has_rgb() ? cloud.rgb.get() : nullptr,
        cloud.has_intensity() ? cloud.intensities.get() : nullptr,
        cloud.has_timestamps() ? cloud.timestamp_offsets.get() : nullptr, *out.points, out.rgb.get(),
        out.intensities.get(), out.timestamp_offsets.get());
    if (!cloud.has_rgb()) out.rgb->clear();
    if (!cloud.has_intensity()) out.intensities->clear();
    if (!cloud.has_timestamps()) out.timestamp_offsets->clear();
    out.covs->clear();
    out.normals->clear();
    const double t0 = cloud.start_time_ms, t1 = cloud.end_time_ms;
    const bool ts = cloud.has_timestamps();
    if (in_place) PointCloudShared::zip(tmp, result, [](const auto& from, auto& to) { to = from; });
    if (ts) { result.start_time_ms = t0; result.end_time_ms = t1; }
}
/// The rows of every attribute a cloud carries, on their way into fresh containers: the rows / dst / bytes table that
/// sp_gather_rows_multi, sp_compact_by_flags_multi and sp_box_filter_compact_multi take, from the attributes `source` has (in
/// PointCloudShared::zip's order: a new attribute is moved once it is listed there), each with a fresh container of `queue` sized
/// for N rows. `points_src`, when given, is read in place of the device copy of the source's points. The caller launches and
/// learns the count M; hand_over() then gives the containers away. Nothing here launches, synchronises or takes scratch memory.
struct RowMover {
    const void* rows[6];
    void* dst[6];
    size_t bytes[6];
    int na = 0;
    RowMover(const sycl_utils::DeviceQueue& queue, const PointCloudShared& source, size_t N, const PointType* points_src = nullptr)
        : source_(source), fresh_(queue) {
        int listed = 0;
        PointCloudShared::zip(source, fresh_, [&](const auto& src, auto& out) {
            const bool is_points = static_cast<const void*>(&src) == &source.points;
            const int i = listed++;
            if (!is_points && !source.has(src)) return;
            moved_ |= 1u << i;
            if (is_points && points_src) rows[na] = points_src;
            else rows[na] = src->device_data();
            dst[na] = out->device_data_for_write(N);
            bytes[na] = sizeof(typename std::remove_reference_t<decltype(*src)>::value_type);
            ++na;
        });
    }
    /// The moved attributes, now M rows each, replace those of `output` (which may be the source). whole_cloud: the attributes the
    /// source lacks become empty containers and the times are the source's; else those attributes and the times stay as they are.
    void hand_over(PointCloudShared& output, size_t M, bool whole_cloud) {
        const double t0 = source_.start_time_ms, t1 = source_.end_time_ms;
        int listed = 0;
        PointCloudShared::zip(fresh_, output, [&](auto& out, auto& to) {
            const bool moved = (moved_ >> listed++) & 1u;
            if (moved) out->set_device_size(M);
            if (moved || whole_cloud) to = out;
        });
        if (whole_cloud) { output.start_time_ms = t0; output.end_time_ms = t1; }
    }

private:
    const PointCloudShared& source_;
    PointCloudShared fresh_;
    unsigned moved_ = 0;  // bit i: zip's i-th attribute is in the table
};
}  // namespace detail

// ================================================================================================ coordinate system
/// common/coordinate_system.hpp:11-26 (REP-103): the frame PolarGrid measures its angles in.
enum class CoordinateSystem : std::uint8_t { LIDAR = 0, CAMERA = 1 };
inline CoordinateSystem coordinate_system_from_string(const std::string& str) {
    std::string upper = str;
    for (auto& c : upper) c = (char)std::toupper((unsigned char)c);
    if (upper == "LIDAR") return CoordinateSystem::LIDAR;
    if (upper == "CAMERA") return CoordinateSystem::CAMERA;
    throw std::invalid_argument("Invalid coordinate system: " + str);
}

// ================================================================================================ robust loss tags
namespace robust {
enum class RobustLossType { NONE, HUBER, TUKEY, CAUCHY, GEMAN_MCCLURE };  // robust/robust.hpp:13-19
inline RobustLossType RobustLossType_from_string(const std::string& str) {
    std::string u = str;
    for (auto& c : u) c = (char)std::toupper((unsigned char)c);
    if (u == "NONE") return RobustLossType::NONE;
    if (u == "HUBER") return RobustLossType::HUBER;
    if (u == "TUKEY") return RobustLossType::TUKEY;
    if (u == "CAUCHY") return RobustLossType::CAUCHY;
    if (u == "GEMAN_MCCLURE") return RobustLossType::GEMAN_MCCLURE;
    throw std::runtime_error("[RobustLossType_from_string] Invalid RobustLossType str '" + str + "'");
}
}  // namespace robust

// ================================================================================================ covariance
namespace covariance {

/// covariance.hpp:260-295
inline sycl_utils::events estimate_async(const sycl_utils::DeviceQueue& queue, const knn::KNNResult& neighbors,
                                         const PointContainerShared& points, CovarianceContainerShared& covs,
                                         const std::vector<sycl_utils::event>& = {}) {
    const size_t N = points.size();
    if (N == 0) { covs.resize(0); return sycl_utils::events(); }
    throw_on_error(sp_cov_estimate(reinterpret_cast<const float*>(points.device_data()), N, neighbors.indices->device_data(),
                                   neighbors.k, reinterpret_cast<float*>(covs.device_data_for_write(N)), queue.stream()));
    return sycl_utils::events(queue.stream());
}
/// covariance.hpp:297-303
inline sycl_utils::events estimate_async(const knn::KNNResult& neighbors, const PointCloudShared& points,
                                         const std::vector<sycl_utils::event>& depends = {}) {
    return estimate_async(points.queue, neighbors, *points.points, *points.covs, depends);
}
/// covariance.hpp:305-311 — search + estimate. With a GridKNN built on `points` the neighbour lists are never written:
/// the self-kNN kernel accumulates the covariance directly (sp_grid_self_knn).
inline sycl_utils::events estimate_async(const knn::KNNBase& knn, const PointCloudShared& points, const size_t k,
                                         const std::vector<sycl_utils::event>& depends = {}) {
    if (const auto* grid = dynamic_cast<const knn::GridKNN*>(&knn)) {
        if (grid->size() == points.size() && k <= 20 && points.size() > 0) {
            detail::DeviceScratch ws(sp_grid_self_workspace_bytes(grid->handle()));
            throw_on_error(sp_grid_self_knn(grid->handle(), k, nullptr, nullptr,
                                            reinterpret_cast<float*>(points.covs->device_data_for_write(points.size())),
                                            nullptr, ws.p, sp_grid_self_workspace_bytes(grid->handle()), points.queue.stream()));
            points.queue.wait();  // the scratch dies with this scope
            return sycl_utils::events(points.queue.stream());
        }
    }
    knn::KNNResult neighbors;
    auto ev = knn.knn_search_async(points, k, neighbors, depends);
    return estimate_async(neighbors, points, ev.evs);
}
/// covariance.hpp:323-381 — M-estimated covariances (K8)
inline sycl_utils::events estimate_robust_async(const sycl_utils::DeviceQueue& queue, const knn::KNNResult& neighbors,
                                                const PointContainerShared& points, CovarianceContainerShared& covs,
                                                robust::RobustLossType robust_type = robust::RobustLossType::CAUCHY,
                                                float mad_scale = 1.0f, float min_robust_scale = 1.0f,
                                                size_t robust_max_iterations = 1,
                                                const std::vector<sycl_utils::event>& = {}) {
    if (neighbors.k > 64) throw std::runtime_error("[covariance::estimate_robust_async] neighbor K is too large. MAX_K is 64");
    const size_t N = points.size();
    if (N == 0) { covs.resize(0); return sycl_utils::events(); }
    throw_on_error(sp_cov_estimate_robust(reinterpret_cast<const float*>(points.device_data()), N,
                                          neighbors.indices->device_data(), neighbors.k, int(robust_type), mad_scale,
                                          min_robust_scale, robust_max_iterations,
                                          reinterpret_cast<float*>(covs.device_data_for_write(N)), queue.stream()));
    return sycl_utils::events(queue.stream());
}
/// covariance.hpp:383-390
inline sycl_utils::events estimate_robust_async(const knn::KNNResult& neighbors, const PointCloudShared& points,
                                                robust::RobustLossType robust_type = robust::RobustLossType::CAUCHY,
                                                float mad_scale = 1.0f, float min_robust_scale = 1.0f,
                                                size_t robust_max_iterations = 1,
                                                const std::vector<sycl_utils::event>& depends = {}) {
    return estimate_robust_async(points.queue, neighbors, *points.points, *points.covs, robust_type, mad_scale,
                                 min_robust_scale, robust_max_iterations, depends);
}
/// covariance.hpp:400-411
inline sycl_utils::events estimate_robust_async(const knn::KNNBase& knn, const PointCloudShared& points,
                                                const size_t k_correspondences,
                                                robust::RobustLossType robust_type = robust::RobustLossType::CAUCHY,
                                                float mad_scale = 1.0f, float min_robust_scale = 1.0f,
                                                size_t robust_max_iterations = 1,
                                                const std::vector<sycl_utils::event>& depends = {}) {
    knn::KNNResult neighbors;
    auto ev = knn.knn_search_async(points, k_correspondences, neighbors, depends);
    return estimate_robust_async(neighbors, points, robust_type, mad_scale, min_robust_scale, robust_max_iterations, ev.evs);
}
/// covariance.hpp:417-443
inline sycl_utils::events estimate_normals_async(const knn::KNNResult& neighbors, const PointCloudShared& points,
                                                 const std::vector<sycl_utils::event>& = {}) {
    const size_t N = points.size();
    if (N == 0) { points.normals->resize(0); return sycl_utils::events(); }
    throw_on_error(sp_normals_from_knn(points.points_device(), N, neighbors.indices->device_data(), neighbors.k,
                                       reinterpret_cast<float*>(points.normals->device_data_for_write(N)), points.queue.stream()));
    return sycl_utils::events(points.queue.stream());
}
/// covariance.hpp:451-459
inline sycl_utils::events estimate_normals_async(const knn::KNNBase& knn, const PointCloudShared& points, const size_t k,
                                                 const std::vector<sycl_utils::event>& depends = {}) {
    knn::KNNResult neighbors;
    auto ev = knn.knn_search_async(points, k, neighbors, depends);
    return estimate_normals_async(neighbors, points, ev.evs);
}
/// covariance.hpp:465-495
inline sycl_utils::events extract_normals_async(const PointCloudShared& points, const std::vector<sycl_utils::event>& = {}) {
    if (!points.has_cov()) throw std::runtime_error("[covariance::extract_normals_async] covariances not computed");
    const size_t N = points.size();
    throw_on_error(sp_normals_from_cov(points.points_device(), points.covs_device(), N,
                                       reinterpret_cast<float*>(points.normals->device_data_for_write(N)), points.queue.stream()));
    return sycl_utils::events(points.queue.stream());
}
inline void extract_normals(const PointCloudShared& points, const std::vector<sycl_utils::event>& depends = {}) {
    extract_normals_async(points, depends).wait_and_throw();
}

}  // namespace covariance

// ================================================================================================ feature (MI355X extension)
namespace feature {
/// FPFH descriptors of a cloud: size() rows of SP_FPFH_STRIDE floats on the device, 33 bins and 3 zeros each.
struct FPFHFeatures {
    shared_vector_ptr<float> rows = nullptr;
    size_t count = 0;
    size_t size() const { return count; }
    const float* device_data() const { return count ? rows->device_data() : nullptr; }
};
/// sp_fpfh_compute on the cloud's stream: `neighbors` is a kNN result of the cloud on itself (k <= SP_FPFH_MAX_K, the point
/// itself may or may not be in its list). The cloud's normals must be of unit length and CONSISTENTLY ORIENTED — what
/// covariance::estimate_normals_async gives a scan whose sensor sits at the origin; the features are signed, a flipped normal is
/// another descriptor. Enqueue only.
inline FPFHFeatures compute_fpfh_async(const knn::KNNResult& neighbors, const PointCloudShared& cloud) {
    FPFHFeatures out;
    out.rows = std::make_shared<shared_vector<float>>(cloud.queue);
    out.count = cloud.size();
    if (out.count == 0) return out;
    if (!cloud.has_normal()) throw std::runtime_error("[feature::compute_fpfh_async] normals not computed");
    if (neighbors.query_size != out.count) throw std::invalid_argument("[feature::compute_fpfh_async] the neighbour lists are not this cloud's");
    hipStream_t st = cloud.queue.stream();
    detail::DeviceScratch ws(sp_fpfh_workspace_bytes(out.count), st);
    ws.stream_ordered = true;
    throw_on_error(sp_fpfh_compute(cloud.points_device(), cloud.normals_device(), out.count, neighbors.indices->device_data(),
                                   neighbors.distances->device_data(), neighbors.k,
                                   out.rows->device_data_for_write(out.count * SP_FPFH_STRIDE), nullptr, nullptr, ws.p, ws.bytes, st));
    return out;
}
inline FPFHFeatures compute_fpfh(const knn::KNNResult& neighbors, const PointCloudShared& cloud) {
    FPFHFeatures out = compute_fpfh_async(neighbors, cloud);
    hip_check(hipStreamSynchronize(cloud.queue.stream()), "sync");
    return out;
}

/// Intensity gradients of a cloud: size() rows (d.x, d.y, d.z, I) on the device, the gradient of the intensity in
/// the point's tangent plane and the intensity itself; (0, 0, 0, NaN) where a point has none.
struct IntensityGradients {
    shared_vector_ptr<float> rows = nullptr;
    size_t count = 0;
    size_t size() const { return count; }
    const float* device_data() const { return count ? rows->device_data() : nullptr; }
};
/// sp_intensity_gradient on the cloud's stream: `neighbors` is a kNN result of the cloud on itself (k >= 2; the point itself is
/// skipped where it is in its list). The cloud needs unit normals and intensities. The gradients are vectors in the frame the
/// cloud is in AT THIS MOMENT: transform the cloud afterwards and they are stale. Enqueue only.
inline IntensityGradients compute_intensity_gradients_async(const knn::KNNResult& neighbors, const PointCloudShared& cloud) {
    IntensityGradients out;
    out.rows = std::make_shared<shared_vector<float>>(cloud.queue);
    out.count = cloud.size();
    if (!cloud.has_normal()) throw std::runtime_error("[feature::compute_intensity_gradients_async] normals not computed");
    if (!cloud.has_intensity()) throw std::runtime_error("[feature::compute_intensity_gradients_async] the cloud has no intensities");
    if (out.count == 0) return out;
    if (neighbors.query_size != out.count)
        throw std::invalid_argument("[feature::compute_intensity_gradients_async] the neighbour lists are not this cloud's");
    throw_on_error(sp_intensity_gradient(cloud.points_device(), cloud.normals_device(), cloud.intensities->device_data(), out.count,
                                         neighbors.indices->device_data(), neighbors.k, out.rows->device_data_for_write(out.count * 4),
                                         cloud.queue.stream()));
    return out;
}
inline IntensityGradients compute_intensity_gradients(const knn::KNNResult& neighbors, const PointCloudShared& cloud) {
    IntensityGradients out = compute_intensity_gradients_async(neighbors, cloud);
    hip_check(hipStreamSynchronize(cloud.queue.stream()), "sync");
    return out;
}
}  // namespace feature

// ================================================================================================ filters
namespace filter {

/// filter/voxel_downsampling.hpp:14-289. Keys, sort and aggregation all run on the device (sp_voxel_downsample).
class VoxelGrid {
public:
    using Ptr = std::shared_ptr<VoxelGrid>;
    VoxelGrid(const sycl_utils::DeviceQueue& queue, const float voxel_size) : queue_(queue) { set_voxel_size(voxel_size); }
    void set_voxel_size(const float voxel_size) {
        if (voxel_size <= 0.0f) throw std::invalid_argument("voxel_size must be positive");
        voxel_size_ = voxel_size;
        voxel_size_inv_ = 1.0f / voxel_size_;
        boxes_.forget();  // the remembered key box is in units of the old voxel size
    }
    float get_voxel_size() const { return voxel_size_; }
    void set_min_voxel_count(const size_t n) { min_voxel_count_ = n; }

    void downsampling(const PointContainerShared& points, PointContainerShared& result) {
        const size_t N = points.size();
        if (N == 0) { result.resize(0); return; }
        run(reinterpret_cast<const float*>(points.device_data()), N, nullptr, nullptr, nullptr, result, nullptr, nullptr, nullptr);
    }
    void downsampling(const PointCloudShared& cloud, PointCloudShared& result) {
        detail::downsample_cloud(queue_, cloud, result, [this](auto&&... io) { run(io...); });
    }

private:
    void run(const float* pts, size_t N, const RGBContainerShared* rgb, const IntensityContainerShared* inten,
             const TimestampContainerShared* ts, PointContainerShared& out_pts, RGBContainerShared* out_rgb,
             IntensityContainerShared* out_inten, TimestampContainerShared* out_ts) {
        hipStream_t st = queue_.stream();
        const std::array<int32_t, 8> h = detail::downsample_run(
            boxes_, st, N, rgb, inten, ts, out_pts, out_rgb, out_inten, out_ts,
            [&](int32_t* box6_dev) { throw_on_error(sp_voxel_key_box(pts, N, voxel_size_inv_, box6_dev, st)); },
            [&](auto... tail) { throw_on_error(sp_voxel_downsample_report(pts, N, voxel_size_inv_, min_voxel_count_, tail...)); });
        if (h[0] != 0 && h[2] <= h[5] && h[3] <= h[6] && h[4] <= h[7]) {
            // every output point is the mean of points of one voxel, so it lies in that voxel; the voxels' key box is h[2..7]
            // (coordinates offset by 2^20, compute_voxel_bit): the cloud's bounding box, a voxel wider on every side against the
            // rounding of floor(p / size), for whoever builds a grid on the cloud next
            float box[6];
            for (int a = 0; a < 3; ++a) {
                box[a] = float(h[2 + a] - (1 << 20) - 1) * voxel_size_;
                box[3 + a] = float(h[5 + a] - (1 << 20) + 2) * voxel_size_;
            }
            ::sycl_points::detail::BoundsHints::put(out_pts.generation(), box);
        }
    }
    sycl_utils::DeviceQueue queue_;
    float voxel_size_ = 1.0f, voxel_size_inv_ = 1.0f;
    size_t min_voxel_count_ = 1;
    detail::KeyBoxMemory boxes_;  // widened key box of the previous clouds (the compressed sort's guess)
};

/// filter/polar_downsampling.hpp:104-452. VoxelGrid's device path with the polar key (sp_polar_downsample_report): keys, sort and
/// aggregation all on the device, where the reference sorts and walks the keys on the host. No bounds hint is left for the
/// output (a box of polar key fields is not a Cartesian box): a grid built on it measures its own bounds.
class PolarGrid {
public:
    using Ptr = std::shared_ptr<PolarGrid>;
    PolarGrid(const sycl_utils::DeviceQueue& queue, float distance_voxel_size, float elevation_voxel_size, float azimuth_voxel_size,
              CoordinateSystem coord = CoordinateSystem::LIDAR)
        : queue_(queue), coord_(coord) {
        if (distance_voxel_size <= 0.0f || elevation_voxel_size <= 0.0f || azimuth_voxel_size <= 0.0f)
            throw std::invalid_argument("voxel sizes must be positive");
        set_distance_voxel_size(distance_voxel_size);
        set_elevation_voxel_size(elevation_voxel_size);
        set_azimuth_voxel_size(azimuth_voxel_size);
    }
    void set_distance_voxel_size(const float size) {
        if (size <= 0.0f) throw std::invalid_argument("distance_voxel_size must be positive");
        distance_voxel_size_ = size;
        distance_voxel_size_inv_ = 1.0f / size;
        boxes_.forget();  // (the remembered key box is in units of the old size)
    }
    float get_distance_voxel_size() const { return distance_voxel_size_; }
    void set_elevation_voxel_size(const float size) {
        if (size <= 0.0f) throw std::invalid_argument("elevation_voxel_size must be positive");
        elevation_voxel_size_ = size;
        elevation_voxel_size_inv_ = 1.0f / size;
        boxes_.forget();
    }
    float get_elevation_voxel_size() const { return elevation_voxel_size_; }
    void set_azimuth_voxel_size(const float size) {
        if (size <= 0.0f) throw std::invalid_argument("azimuth_voxel_size must be positive");
        azimuth_voxel_size_ = size;
        azimuth_voxel_size_inv_ = 1.0f / size;
        boxes_.forget();
    }
    float get_azimuth_voxel_size() const { return azimuth_voxel_size_; }
    void set_min_voxel_count(const size_t min_voxel_count) { min_voxel_count_ = min_voxel_count; }
    size_t get_min_voxel_count() const { return min_voxel_count_; }
    void set_coordinate_system(const CoordinateSystem coord) {
        coord_ = coord;
        boxes_.forget();
    }
    CoordinateSystem get_coordinate_system() const { return coord_; }

    /// polar_downsampling.hpp:200-209 (in place allowed)
    void downsampling(const PointContainerShared& points, PointContainerShared& result) {
        const size_t N = points.size();
        if (N == 0) { result.resize(0); return; }
        // in place: the points are read again by a redo (a scan that left the remembered key box), so they are read from a copy
        const bool in_place = &points == &result;
        hipStream_t st = queue_.stream();
        detail::DeviceScratch copy(in_place ? N * sizeof(PointType) : 0, st);
        const float* src = reinterpret_cast<const float*>(points.device_data());
        if (in_place) {
            hip_check(hipMemcpyAsync(copy.p, src, N * sizeof(PointType), hipMemcpyDeviceToDevice, st), "D2D");
            copy.stream_ordered = true;
            src = static_cast<const float*>(copy.p);
        }
        run(src, N, nullptr, nullptr, nullptr, result, nullptr, nullptr, nullptr);
    }
    /// polar_downsampling.hpp:217-236 (in place allowed; start / end time kept when the cloud has timestamps)
    void downsampling(const PointCloudShared& cloud, PointCloudShared& result) {
        detail::downsample_cloud(queue_, cloud, result, [this](auto&&... io) { run(io...); });
    }

private:
    void run(const float* pts, size_t N, const RGBContainerShared* rgb, const IntensityContainerShared* inten,
             const TimestampContainerShared* ts, PointContainerShared& out_pts, RGBContainerShared* out_rgb,
             IntensityContainerShared* out_inten, TimestampContainerShared* out_ts) {
        hipStream_t st = queue_.stream();
        const int coord = static_cast<int>(coord_);
        detail::downsample_run(
            boxes_, st, N, rgb, inten, ts, out_pts, out_rgb, out_inten, out_ts,
            [&](int32_t* box6_dev) {
                throw_on_error(sp_polar_key_box(pts, N, coord, distance_voxel_size_inv_, elevation_voxel_size_inv_,
                                                azimuth_voxel_size_inv_, box6_dev, st));
            },
            [&](auto... tail) {
                throw_on_error(sp_polar_downsample_report(pts, N, coord, distance_voxel_size_inv_, elevation_voxel_size_inv_,
                                                          azimuth_voxel_size_inv_, min_voxel_count_, tail...));
            });
    }
    sycl_utils::DeviceQueue queue_;
    float distance_voxel_size_ = 1.0f, elevation_voxel_size_ = 1.0f, azimuth_voxel_size_ = 1.0f;
    float distance_voxel_size_inv_ = 1.0f, elevation_voxel_size_inv_ = 1.0f, azimuth_voxel_size_inv_ = 1.0f;
    size_t min_voxel_count_ = 1;
    CoordinateSystem coord_;
    detail::KeyBoxMemory boxes_;  // widened key box of the previous clouds (the compressed sort's guess)
};

/// common/filter_by_flags.hpp:15-99 — stable compaction on the device (sp_compact_by_flags).
class FilterByFlags {
public:
    using Ptr = std::shared_ptr<FilterByFlags>;
    explicit FilterByFlags(const sycl_utils::DeviceQueue& queue) : queue_(queue) {}

    template <typename T>
    void filter_by_flags(const shared_vector<T>& source, shared_vector<T>& output, const shared_vector<uint8_t>& flags) const {
        const size_t N = source.size();
        if (N == 0) return;
        const size_t ws_bytes = sp_compact_workspace_bytes(N);
        hipStream_t st = queue_.stream();
        detail::DeviceScratch ws(ws_bytes, st), count(4, st), tmp(N * sizeof(T), st);
        throw_on_error(sp_compact_by_flags(source.device_data(), N, sizeof(T), flags.device_data(), tmp.p, nullptr,
                                           static_cast<uint32_t*>(count.p), ws.p, ws_bytes, st));
        const size_t M = detail::read_u32(count.p, st);
        T* dst = output.device_data_for_write(std::max<size_t>(M, 1));
        if (M) hip_check(hipMemcpyAsync(dst, tmp.p, M * sizeof(T), hipMemcpyDeviceToDevice, st), "D2D");
        hip_check(hipStreamSynchronize(st), "sync");
        output.set_device_size(M);
    }
    template <typename T>
    void filter_by_flags(shared_vector<T>& data, const shared_vector<uint8_t>& flags) const { filter_by_flags(data, data, flags); }

    void calculate_indices(const shared_vector<uint8_t>& flags, shared_vector<int32_t>& indices) const {
        const size_t N = flags.size();
        if (N == 0) return;
        const size_t ws_bytes = sp_compact_workspace_bytes(N);
        detail::DeviceScratch ws(ws_bytes, queue_.stream()), count(4, queue_.stream());
        throw_on_error(sp_compact_by_flags(flags.device_data(), N, 0 + 4 * 0 + 4, flags.device_data(), nullptr,
                                           indices.device_data_for_write(N), static_cast<uint32_t*>(count.p), ws.p, ws_bytes,
                                           queue_.stream()));
        queue_.wait();
    }

private:
    sycl_utils::DeviceQueue queue_;
};

/// filter/preprocess_filter.hpp — the operators the hot path's callers use (box filter, random sampling, farthest point sampling).
class PreprocessFilter {
public:
    using Ptr = std::shared_ptr<PreprocessFilter>;
    explicit PreprocessFilter(const sycl_utils::DeviceQueue& queue) : queue_(queue), mt_(1234), fps_mt_(1234), weighted_mt_(1234), mixed_mt_(1234) {
        flags_ = std::make_shared<shared_vector<uint8_t>>(queue);
    }
    /// preprocess_filter.hpp:46-51: every sampling operator has a generator of its own; the call seeds them all
    void set_random_seed(uint_fast32_t seed) { mt_.seed(seed); fps_mt_.seed(seed); weighted_mt_.seed(seed); mixed_mt_.seed(seed); }

    /// preprocess_operator/box_filter_operator.hpp:24-54 (K10 on the device, compaction on the device)
    void box_filter(const PointCloudShared& source, PointCloudShared& output, float min_distance = 1.0f,
                    float max_distance = std::numeric_limits<float>::max()) {
        const size_t N = source.size();
        if (N == 0) return;
        // the box test, the scan of its flags and the move of every attribute's kept rows in one launch (sp_box_filter_compact_multi)
        box_ = BoxArgs{true, min_distance, max_distance};
        apply_flags(source, output);
        box_.on = false;
    }
    void box_filter(PointCloudShared& data, float min_distance = 1.0f, float max_distance = std::numeric_limits<float>::max()) {
        box_filter(data, data, min_distance, max_distance);
    }
    /// preprocess_operator/random_sampling_operator.hpp:24-51 — host partial Fisher-Yates with std::mt19937
    void random_sampling(const PointCloudShared& source, PointCloudShared& output, size_t sampling_num) {
        const size_t N = source.size();
        if (N <= sampling_num) {
            if (&source != &output) output = PointCloudShared(source);
            return;
        }
        std::vector<size_t> indices(N);
        std::iota(indices.begin(), indices.end(), 0);
        for (size_t i = 0; i < sampling_num; ++i) {
            std::uniform_int_distribution<size_t> dist(i, N - 1);
            std::swap(indices[i], indices[dist(mt_)]);
        }
        // The reference sets a flag per drawn index and filters every attribute by the flags: the sample in the cloud's own order.
        // The same rows by their (sorted) indices: 4 KB up, ONE gather launch for all attributes — no scan of the whole cloud's
        // flags, no launch per attribute, no count to read back.
        std::vector<uint32_t> picked(sampling_num);
        for (size_t i = 0; i < sampling_num; ++i) picked[i] = static_cast<uint32_t>(indices[i]);
        std::sort(picked.begin(), picked.end());
        gather_rows(source, output, picked);
    }
    void random_sampling(PointCloudShared& data, size_t sampling_num) { random_sampling(data, data, sampling_num); }
    /// preprocess_operator/farthest_point_sampling_operator.hpp:27-91. The first index is the reference's draw from the
    /// operator's own mt19937 (fps_mt_); the chain of argmax decisions runs on the device (sp_farthest_point_sampling: the
    /// reference goes back to the host once per sample); the kept rows, in the cloud's own order, move through the flags path.
    /// Kept from the reference: N <= sampling_num copies the source (an empty one too); sampling_num == 0 keeps the one random
    /// first point; duplicates and NaN points select an index again, so fewer than sampling_num points may come out. Time
    /// stamps follow filter_by_flags (preprocess_filter.hpp:198-227): end = start + the largest kept offset; a cloud without
    /// offsets gets start = end = 0.
    void farthest_point_sampling(const PointCloudShared& source, PointCloudShared& output, size_t sampling_num) {
        const size_t N = source.size();
        if (N <= sampling_num) {
            if (&source != &output) output = PointCloudShared(source);
            return;
        }
        std::uniform_int_distribution<size_t> dist(0, N - 1);
        const uint32_t first = static_cast<uint32_t>(dist(fps_mt_));
        const size_t S = std::max<size_t>(sampling_num, 1);  // (the reference's loop starts at 1: sampling_num 0 keeps the first)
        hipStream_t st = queue_.stream();
        const size_t ws_bytes = sp_fps_workspace_bytes(N, S);
        detail::DeviceScratch ws(ws_bytes, st), order(S * sizeof(uint32_t), st);
        ws.stream_ordered = order.stream_ordered = true;  // (used on st only)
        auto run = [&] {
            throw_on_error(sp_farthest_point_sampling(reinterpret_cast<const float*>(source.points->device_data()), N, S, first,
                                                      static_cast<uint32_t*>(order.p), flags_->device_data_for_write(N), nullptr,
                                                      ws.p, ws_bytes, st));
            return sp_fps_status(ws.p, st);
        };
        // a persistent launch whose bounded wait ran out leaves the sample incomplete: the library then takes the per-sample form
        int rc = run();
        if (rc == SP_ERR_RUNTIME) rc = run();
        throw_on_error(rc);
        apply_flags(source, output);
        sampled_time_range(output);
    }
    void farthest_point_sampling(PointCloudShared& data, size_t sampling_num) { farthest_point_sampling(data, data, sampling_num); }
    /// preprocess_operator/weighted_sampling_operator.hpp:29-95 — Efraimidis-Spirakis without replacement. The reference's host loop
    /// over every point (a log, a draw and a heap step each) is the device's here (sp_weight_check, sp_weighted_sample_flags); the
    /// host only draws, one per positive weight, from the operator's own generator (weighted_mt_), and reads two words back. The
    /// checks, their order and their texts are the reference's. The kept rows move through the flags path with the count known.
    void weighted_random_sampling(const PointCloudShared& source, PointCloudShared& output, const shared_vector<float>& weights,
                                  size_t sampling_num) {
        const size_t N = source.size();
        if (N <= sampling_num) {
            if (&source != &output) output = PointCloudShared(source);
            return;
        }
        if (weights.size() != N)
            throw std::invalid_argument("[PreprocessFilter::weighted_random_sampling] weights size must match points");
        hipStream_t st = queue_.stream();
        const float* const w = weights.device_data();
        const WeightReport rep = check_weights(w, N, st);
        if (rep.first_invalid != kNoInvalidWeight)
            throw std::invalid_argument("[PreprocessFilter::weighted_random_sampling] weights must be finite and non-negative");
        if (rep.positive == 0)
            throw std::invalid_argument("[PreprocessFilter::weighted_random_sampling] at least one weight must be positive");
        if (sampling_num > rep.positive)
            throw std::invalid_argument("[PreprocessFilter::weighted_random_sampling] sampling_num exceeds positive-weight points");
        weighted_flags(w, N, sampling_num, rep.positive, weighted_mt_, st);
        apply_flags(source, output, sampling_num);
        sampled_time_range(output);
    }
    void weighted_random_sampling(PointCloudShared& data, const shared_vector<float>& weights, size_t sampling_num) {
        weighted_random_sampling(data, data, weights, sampling_num);
    }
    /// preprocess_operator/mixed_random_sampling_operator.hpp:28-105 — floor(sampling_num * weighted_ratio) points by their weights
    /// (as above, on mixed_mt_; fewer positive weights than that: all of them), the rest uniformly among the others: the
    /// reference's partial Fisher-Yates over the list of unselected indices draws from the same generator afterwards. The host
    /// runs it on POSITIONS in that list (a sparse map of the swapped slots, not N entries); the device finds the point each
    /// position stands for (sp_uniform_fill_flags). weighted_ratio == 0 draws what random_sampling draws with the same seed.
    void mixed_random_sampling(const PointCloudShared& source, PointCloudShared& output, const shared_vector<float>& weights,
                               size_t sampling_num, float weighted_ratio) {
        const size_t N = source.size();
        if (N <= sampling_num) {
            if (&source != &output) output = PointCloudShared(source);
            return;
        }
        if (weights.size() != N) throw std::invalid_argument("[PreprocessFilter::mixed_random_sampling] weights size must match points");
        if (!std::isfinite(weighted_ratio) || weighted_ratio < 0.0f || weighted_ratio > 1.0f)
            throw std::invalid_argument("[PreprocessFilter::mixed_random_sampling] weighted_ratio must be within [0.0, 1.0]");
        // the share drawn by weight: floor of the product in double (:44-45)
        const size_t by_weight = static_cast<size_t>(std::floor(double(sampling_num) * double(weighted_ratio)));
        hipStream_t st = queue_.stream();
        const float* const w = weights.device_data();
        const WeightReport rep = check_weights(w, N, st);
        if (rep.first_invalid != kNoInvalidWeight) {
            // the reference meets the weight inside its loop (:57-62): the positive weights before it have taken their draws
            if (by_weight != 0 && rep.first_invalid != 0) draw_weighted(check_weights(w, rep.first_invalid, st).positive, mixed_mt_);
            throw std::invalid_argument("[PreprocessFilter::mixed_random_sampling] weights must be finite and non-negative");
        }
        // (by_weight == 0 consumes no draw, :63; fewer positive weights than the target: all are kept, all have drawn)
        const size_t selected = std::min(by_weight, rep.positive);
        if (selected != 0) weighted_flags(w, N, by_weight, rep.positive, mixed_mt_, st);
        else hip_check(hipMemsetAsync(flags_->device_data_for_write(N), 0, N, st), "memset");
        const size_t R = N - selected, U = std::min(sampling_num - selected, R);
        if (U != 0) {
            std::unordered_map<size_t, size_t> moved;  // the slots of `remaining` that a swap has touched
            moved.reserve(2 * U);
            auto at = [&](size_t k) { const auto it = moved.find(k); return it == moved.end() ? k : it->second; };
            std::vector<uint32_t> positions(U);
            for (size_t i = 0; i < U; ++i) {
                std::uniform_int_distribution<size_t> dist(i, R - 1);
                const size_t j = dist(mixed_mt_);
                const size_t vi = at(i), vj = at(j);
                moved[i] = vj;
                moved[j] = vi;
                positions[i] = static_cast<uint32_t>(vj);
            }
            std::sort(positions.begin(), positions.end());
            const size_t ws_bytes = sp_uniform_fill_workspace_bytes(N);
            detail::DeviceScratch ws(ws_bytes, st), pos(U * sizeof(uint32_t), st);
            ws.stream_ordered = pos.stream_ordered = true;  // (used on st only)
            hip_check(hipMemcpyAsync(pos.p, positions.data(), U * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D");  // (pageable: staged before the call returns)
            throw_on_error(sp_uniform_fill_flags(flags_->device_data_for_write(N), N, static_cast<const uint32_t*>(pos.p), U, ws.p,
                                                 ws_bytes, st));
        }
        apply_flags(source, output, selected + U);
        sampled_time_range(output);
    }
    void mixed_random_sampling(PointCloudShared& data, const shared_vector<float>& weights, size_t sampling_num, float weighted_ratio) {
        mixed_random_sampling(data, data, weights, sampling_num, weighted_ratio);
    }
    /// preprocess_filter.hpp:147-160, 276-279 + preprocess_operator/angle_incidence_filter_operator.hpp:23-110: the flags on the
    /// device (sp_angle_incidence_flags: the cloud's normals, else extract_normal of its covariances), then every attribute through
    /// the flags path on the same stream: nothing waits in between, one count is read back. An empty source returns before any
    /// check and leaves the output as it is; the checks and their texts are the reference's (the library reports them).
    void angle_incidence_filter(const PointCloudShared& source, PointCloudShared& output, float min_angle, float max_angle) {
        const size_t N = source.size();
        if (N == 0) return;
        throw_on_error(sp_angle_incidence_flags(source.points_device(), source.normals_device(), source.covs_device(), N, min_angle,
                                                max_angle, flags_->device_data_for_write(N), queue_.stream()));
        apply_flags(source, output);
    }
    void angle_incidence_filter(PointCloudShared& data, float min_angle, float max_angle) {
        angle_incidence_filter(data, data, min_angle, max_angle);
    }

private:
    /// filter_by_flags' time stamps (preprocess_filter.hpp:211-224): end = start + the largest kept offset; none: start = end = 0
    static void sampled_time_range(PointCloudShared& output) {
        if (output.has_timestamps()) {
            const auto& off = *output.timestamp_offsets;
            output.end_time_ms = off.empty() ? output.start_time_ms
                                             : output.start_time_ms + static_cast<double>(*std::max_element(off.begin(), off.end()));
        } else {
            output.start_time_ms = 0.0;
            output.end_time_ms = 0.0;
        }
    }
    static constexpr size_t kNoInvalidWeight = 0xffffffffu;
    struct WeightReport { size_t positive, first_invalid; };
    /// sp_weight_check over the first n weights and its two words read back (it synchronises the stream)
    WeightReport check_weights(const float* w, size_t n, hipStream_t st) {
        detail::DeviceScratch report(8, st);
        throw_on_error(sp_weight_check(w, n, static_cast<uint32_t*>(report.p), st));
        uint32_t local[2];
        void* const pinned = detail::pinned_block_4k();  // (a copy into pageable memory is staged inside the runtime)
        uint32_t* const h = pinned ? static_cast<uint32_t*>(pinned) : local;
        hip_check(hipMemcpyAsync(h, report.p, 8, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        return WeightReport{h[0], h[1]};
    }
    /// `count` draws of the weighted part, in the reference's order (one per positive weight, index ascending)
    void draw_weighted(size_t count, std::mt19937& mt) {
        std::uniform_real_distribution<float> dist(std::numeric_limits<float>::min(), 1.0f);
        draws_.resize(count);
        for (size_t j = 0; j < count; ++j) draws_[j] = dist(mt);
    }
    /// flags_ = the m points of the largest keys (all `positive` ones when there are fewer), with `positive` fresh draws of mt
    void weighted_flags(const float* w, size_t N, size_t m, size_t positive, std::mt19937& mt, hipStream_t st) {
        draw_weighted(positive, mt);
        const size_t ws_bytes = sp_weighted_sample_workspace_bytes(N);
        detail::DeviceScratch ws(ws_bytes, st), u(positive * sizeof(float), st);
        ws.stream_ordered = u.stream_ordered = true;  // (used on st only)
        hip_check(hipMemcpyAsync(u.p, draws_.data(), positive * sizeof(float), hipMemcpyHostToDevice, st), "H2D");  // (pageable: staged before the call returns)
        throw_on_error(sp_weighted_sample_flags(w, static_cast<const float*>(u.p), N, m, flags_->device_data_for_write(N), nullptr,
                                                ws.p, ws_bytes, st));
    }
    /// output = the rows `picked` of every attribute of source (sp_gather_rows_multi)
    void gather_rows(const PointCloudShared& source, PointCloudShared& output, const std::vector<uint32_t>& picked) {
        const size_t M = picked.size();
        detail::RowMover mv(queue_, source, M);
        hipStream_t st = queue_.stream();
        size_t got = 0;
        void* idx = ::sycl_points::detail::DeviceBufferCache::acquire(std::max<size_t>(M, 1) * 4, &got, st);
        hipError_t e = hipMemcpyAsync(idx, picked.data(), M * 4, hipMemcpyHostToDevice, st);  // (pageable: staged before the call returns)
        int rc = SP_OK;
        if (e == hipSuccess) rc = sp_gather_rows_multi(mv.rows, mv.bytes, mv.dst, mv.na, static_cast<const uint32_t*>(idx), M, st);
        ::sycl_points::detail::DeviceBufferCache::release(idx, got, st);
        hip_check(e, "H2D");
        throw_on_error(rc);
        mv.hand_over(output, M, /*whole_cloud=*/true);
    }
    void apply_flags(const PointCloudShared& source, PointCloudShared& output, size_t known_count = SIZE_MAX) {
        // FilterByFlags over every attribute the cloud carries (preprocess_operator_base): one scan of the flags, one
        // compaction launch per attribute, written straight into the new containers (no staging copy), ONE count read-back.
        const size_t N = source.size();
        // the box filter reads the points once: straight out of the pinned host copy when that is the current one (a fresh scan)
        bool pts_in_place = false;
        const PointType* const pts = box_.on ? source.points->device_readable_once(&pts_in_place) : source.points->device_data();
        detail::RowMover mv(queue_, source, N, pts);
        const size_t ws_bytes = sp_compact_workspace_bytes(N);
        hipStream_t st = queue_.stream();
        hipStream_t ws_release_stream = nullptr;
        // (with a known count nothing synchronises here: the scratch goes back tagged with the stream's event instead of idle)
        struct Scratch {
            void* p = nullptr; size_t bytes = 0; hipStream_t* tag;
            Scratch(size_t n, hipStream_t* t, hipStream_t use) : tag(t) { if (n) p = ::sycl_points::detail::DeviceBufferCache::acquire(n, &bytes, use); }
            ~Scratch() {
                if (!p) return;
                if (std::uncaught_exceptions() > 0) (void)hipDeviceSynchronize();  // (left by an exception: nothing was waited for)
                ::sycl_points::detail::DeviceBufferCache::release(p, bytes, *tag, *tag == nullptr);
            }
        } ws(ws_bytes, &ws_release_stream, st), count(4, &ws_release_stream, st);
        // the count comes through a host-mapped word the kernel stores to (no copy, no synchronisation) when one is to be had
        const detail::MappedWord& mapped = detail::MappedWord::mine();
        const bool poll = known_count == SIZE_MAX && mapped.usable();
        uint32_t* const count_dev = poll ? mapped.dev : static_cast<uint32_t*>(count.p);
        if (poll) mapped.arm();
        if (box_.on) {
            const int rc = sp_box_filter_compact_multi(reinterpret_cast<const float*>(pts), N, box_.min_distance, box_.max_distance,
                                                       mv.rows, mv.bytes, mv.dst, mv.na, flags_->device_data_for_write(N), nullptr,
                                                       count_dev, ws.p, ws_bytes, st);
            if (pts_in_place) source.points->host_read_enqueued(st);
            throw_on_error(rc);
        } else
            throw_on_error(sp_compact_by_flags_multi(mv.rows, mv.bytes, mv.dst, mv.na, N, flags_->device_data(), nullptr, count_dev,
                                                     ws.p, ws_bytes, st));
        size_t M = known_count;
        if (poll) { M = mapped.wait(st); ws_release_stream = st; }  // (nothing synchronised: the scratch goes back behind the stream's work)
        else if (known_count == SIZE_MAX) M = detail::read_u32(count.p, st);  // (synchronises: the scratch is idle when it leaves scope)
        else ws_release_stream = st;
        mv.hand_over(output, M, /*whole_cloud=*/true);
    }
    struct BoxArgs { bool on = false; float min_distance = 0.0f, max_distance = 0.0f; } box_;  // apply_flags makes the flags itself
    sycl_utils::DeviceQueue queue_;
    shared_vector_ptr<uint8_t> flags_;
    std::mt19937 mt_;
    std::mt19937 fps_mt_;  // farthest point sampling's own generator (preprocess_filter.hpp:46-51)
    std::mt19937 weighted_mt_, mixed_mt_;  // and the weighted and the mixed sampler's
    std::vector<float> draws_;             // the weighted draws of the current call (its capacity is kept)
};

/// filter/outlier_removal_filter.hpp:13-242. The kNN search is the caller's KDTree as it is; the flags come from
/// sp_outlier_statistical_flags (three launches, no wait in between: the reference waits after each of its three kernels and reads a
/// USM word on the host twice) or sp_outlier_radius_flags on the same stream, and every attribute the reference moves (:224-241)
/// goes through ONE sp_compact_by_flags_multi, which also leaves the new indices calculate_indices() returns. One count is read back.
/// Kept from the reference: the squared neighbour distances are averaged and compared as they are, radius() compares the squared
/// distance with `radius` itself (:178-188), too few points print its message and leave the cloud untouched. mean_k == 0 on a
/// non-empty cloud is std::invalid_argument here (the reference divides by zero and keeps every point).
class OutlierRemoval {
public:
    using Ptr = std::shared_ptr<OutlierRemoval>;
    explicit OutlierRemoval(const sycl_utils::DeviceQueue& queue) : queue_(queue), filter_(queue) {
        flags_ = std::make_shared<shared_vector<uint8_t>>(queue);
        indices_ = std::make_shared<shared_vector<int32_t>>(queue);
        local_mean_distance_ = std::make_shared<shared_vector<float>>(queue);
        stats_ = std::make_shared<shared_vector<float>>(queue);
        neighbors_ = std::make_shared<knn::KNNResult>();
    }

    /// :38-145 — a point is removed when the mean of its mean_k squared neighbour distances is above
    /// global mean + stddev_mul_thresh * global standard deviation of those means
    void statistical(PointCloudShared& cloud, knn::KDTree& tree, size_t mean_k, float stddev_mul_thresh, bool remove_from_tree = false) {
        const size_t N = cloud.size();
        if (N < mean_k) {
            std::cerr << "Not enough points in the cloud [ points = " << N << ", mean_k = " << mean_k << " ]" << std::endl;
            return;
        }
        if (N == 0) return;
        hipStream_t st = queue_.stream();
        tree.knn_search_async(cloud, mean_k, *neighbors_);
        const size_t ws_bytes = sp_outlier_workspace_bytes(N);
        detail::DeviceScratch ws(ws_bytes, st);
        throw_on_error(sp_outlier_statistical_flags(neighbors_->distances->device_data(), N, mean_k, mean_k, stddev_mul_thresh,
                                                    flags_->device_data_for_write(N), local_mean_distance_->device_data_for_write(N),
                                                    stats_->device_data_for_write(4), ws.p, ws_bytes, st));
        filter_by_flags(cloud);  // (synchronises: the scratch is idle when it leaves scope)
        if (remove_from_tree) tree.remove_nodes_by_flags(get_flags(), calculate_indices());
    }

    /// :155-199 — a point is removed when its min_k-th neighbour other than itself is farther than `radius` (compared as the
    /// reference compares: the squared distance against the radius)
    void radius(PointCloudShared& cloud, knn::KDTree& tree, size_t min_k, float radius, bool remove_from_tree = false) {
        const size_t N = cloud.size();
        if (N < min_k) {
            std::cerr << "Not enough points in the cloud [ points = " << N << ", min_k = " << min_k << " ]" << std::endl;
            return;
        }
        if (N == 0) return;
        tree.knn_search_async(cloud, min_k + 1, *neighbors_);  // (the tree holds the point itself: :162-163)
        throw_on_error(sp_outlier_radius_flags(neighbors_->distances->device_data(), N, min_k + 1, min_k, radius,
                                               flags_->device_data_for_write(N), queue_.stream()));
        filter_by_flags(cloud);
        if (remove_from_tree) tree.remove_nodes_by_flags(get_flags(), calculate_indices());
    }

    /// INCLUDE_FLAG for the points of the last call that stayed, REMOVE_FLAG for the others (:203)
    const shared_vector<uint8_t>& get_flags() const { return *flags_; }
    /// the new index of every point of the last call, -1 for a removed one (:208-211): left by the compaction itself
    const shared_vector<int32_t>& calculate_indices() const {
        if (indices_->size() != flags_->size()) filter_.calculate_indices(*flags_, *indices_);
        return *indices_;
    }
    /// MI355X extension: the statistical filter's per-point means of the last call, and {global mean, variance, threshold, n}
    const shared_vector<float>& get_local_mean_distance() const { return *local_mean_distance_; }
    const shared_vector<float>& get_statistics() const { return *stats_; }

private:
    /// :224-241 — covariances, normals, colours, intensities, time stamps and points by flags_: one scan, one launch per attribute
    void filter_by_flags(PointCloudShared& data) {
        const size_t N = data.size();
        hipStream_t st = queue_.stream();
        detail::RowMover mv(queue_, data, N);
        const size_t ws_bytes = sp_compact_workspace_bytes(N);
        detail::DeviceScratch ws(ws_bytes, st), count(4, st);
        throw_on_error(sp_compact_by_flags_multi(mv.rows, mv.bytes, mv.dst, mv.na, N, flags_->device_data(),
                                                 indices_->device_data_for_write(N), static_cast<uint32_t*>(count.p), ws.p, ws_bytes, st));
        const size_t M = detail::read_u32(count.p, st);
        mv.hand_over(data, M, /*whole_cloud=*/false);  // (the attributes the cloud lacks and its times stay)
    }

    sycl_utils::DeviceQueue queue_;
    FilterByFlags filter_;
    knn::KNNResult::Ptr neighbors_;
    shared_vector_ptr<uint8_t> flags_;
    shared_vector_ptr<int32_t> indices_;
    shared_vector_ptr<float> local_mean_distance_;
    shared_vector_ptr<float> stats_;
};

}  // namespace filter

// ================================================================================================ intensity filters
namespace intensity_correction {

/// filter/intensity_correction.hpp:50-135, in place (sp_intensity_correct: the reference's checks in its order and their texts)
inline void correct_intensity(PointCloudShared& cloud, float exponent = 2.0f, float scale = 1.0f, float min_intensity = 0.0f,
                              float max_intensity = 1000.0f, float ref_distance = 1.0f, float angle_exponent = 0.0f) {
    const size_t N = cloud.size();
    if (N == 0) return;
    float* const inten = cloud.has_intensity() ? cloud.intensities->device_data_rw() : nullptr;
    if (inten) cloud.intensities->set_device_size(N);
    throw_on_error(sp_intensity_correct(cloud.points_device(), cloud.normals_device(), cloud.covs_device(), inten, N, exponent, scale,
                                        min_intensity, max_intensity, ref_distance, angle_exponent, cloud.queue.stream()));
    cloud.queue.wait();
}

}  // namespace intensity_correction

namespace detail {
/// smooth_intensity / normalize: a fresh intensity vector written by sp_intensity_gaussian and swapped into the cloud
/// (intensity_gaussian.hpp:116-150, intensity_local_mean_norm.hpp:76-112); mean_min <= 0 selects the smoothing
inline void intensity_gaussian_swap(PointCloudShared& cloud, const knn::KNNResult& neighbors, float sigma_azimuth,
                                    float sigma_elevation, float sigma_range, float mean_min, size_t k_limit) {
    const size_t N = cloud.size();
    const size_t k_stride = neighbors.k;
    const size_t k_use = (k_limit > 0 && k_limit < k_stride) ? k_limit : k_stride;
    const bool usable = cloud.has_intensity() && k_stride >= 1;  // (otherwise the library reports what is missing)
    auto tmp = std::make_shared<IntensityContainerShared>(cloud.queue);
    throw_on_error(sp_intensity_gaussian(cloud.points_device(), cloud.has_intensity() ? cloud.intensities->device_data() : nullptr,
                                         usable && neighbors.indices ? neighbors.indices->device_data() : nullptr, N, k_stride, k_use,
                                         sigma_azimuth, sigma_elevation, sigma_range, mean_min,
                                         usable ? tmp->device_data_for_write(N) : nullptr, cloud.queue.stream()));
    cloud.queue.wait();
    std::swap(cloud.intensities, tmp);
}
}  // namespace detail

namespace intensity_gaussian {

/// filter/intensity_gaussian.hpp:88-151
inline void smooth_intensity(PointCloudShared& cloud, const knn::KNNResult& neighbors, float sigma_azimuth, float sigma_elevation,
                             float sigma_range = 0.05f, size_t k_limit = 0) {
    if (cloud.size() == 0) return;
    detail::intensity_gaussian_swap(cloud, neighbors, sigma_azimuth, sigma_elevation, sigma_range, 0.0f, k_limit);
}

}  // namespace intensity_gaussian

namespace intensity_local_mean_norm {

/// filter/intensity_local_mean_norm.hpp:36-113
inline void normalize(PointCloudShared& cloud, const knn::KNNResult& neighbors, float sigma_azimuth, float sigma_elevation,
                      float sigma_range = 0.05f, float mean_min = 1e-3f, size_t k_limit = 0) {
    if (cloud.size() == 0) return;
    if (mean_min <= 0.0f) {  // the last of the reference's checks (:72-74); the ones before it are the library's, in its order
        if (cloud.has_intensity() && neighbors.k >= 1 && !(sigma_azimuth <= 0.0f || sigma_elevation <= 0.0f || sigma_range <= 0.0f))
            throw std::runtime_error("[intensity_local_mean_norm::normalize] mean_min must be positive");
        mean_min = 1.0f;  // (selects the normalisation's texts)
    }
    detail::intensity_gaussian_swap(cloud, neighbors, sigma_azimuth, sigma_elevation, sigma_range, mean_min, k_limit);
}

}  // namespace intensity_local_mean_norm

namespace intensity_zscore {

/// filter/intensity_zscore.hpp:40-72 — cloud.intensities replaced by (I - local mean) / local sigma over the neighbours of
/// `neighbors` (0 where sigma < sigma_min): a fresh vector written by sp_intensity_zscore and swapped in. The reference's checks, in
/// its order and with its texts, are the library's; an empty cloud returns before them.
inline void compute(PointCloudShared& cloud, const knn::KNNResult& neighbors, float sigma_min = 0.01f) {
    const size_t N = cloud.size();
    if (N == 0) return;
    const size_t k = neighbors.k;
    const bool usable = cloud.has_intensity() && k >= 3 && neighbors.indices;  // (otherwise the library reports what is missing)
    auto tmp = std::make_shared<IntensityContainerShared>(cloud.queue);
    throw_on_error(sp_intensity_zscore(cloud.has_intensity() ? cloud.intensities->device_data() : nullptr,
                                       usable ? neighbors.indices->device_data() : nullptr, N, k, k, sigma_min,
                                       usable ? tmp->device_data_for_write(N) : nullptr, cloud.queue.stream()));
    cloud.queue.wait();
    std::swap(cloud.intensities, tmp);
}

}  // namespace intensity_zscore

// ================================================================================================ transform
namespace transform {

/// common/transform.hpp:45-94
inline sycl_utils::events transform_async(PointCloudShared& cloud, const TransformMatrix& trans) {
    const size_t N = cloud.size();
    if (N == 0) return sycl_utils::events();
    const bool c = cloud.has_cov(), n = cloud.has_normal();
    float* cv = c ? reinterpret_cast<float*>(cloud.covs->device_data_rw()) : nullptr;
    float* nr = n ? reinterpret_cast<float*>(cloud.normals->device_data_rw()) : nullptr;
    float* pt = reinterpret_cast<float*>(cloud.points->device_data_rw());
    throw_on_error(sp_transform(pt, cv, nr, N, trans.data(), pt, cv, nr, cloud.queue.stream()));
    return sycl_utils::events(cloud.queue.stream());
}
inline void transform(PointCloudShared& cloud, const TransformMatrix& trans) { transform_async(cloud, trans).wait_and_throw(); }
/// common/transform.hpp:107-147
inline PointCloudShared transform_copy(const PointCloudShared& cloud, const TransformMatrix& trans) {
    PointCloudShared ret(cloud);
    transform(ret, trans);
    return ret;
}

}  // namespace transform
}  // namespace algorithms
}  // namespace sycl_points
