// sycl_points facade for MI355X — Scan Context place recognition (MI355X extension; the reference has nothing of
// the kind): "have I been here before, and at what heading?" — the link between the odometry loops and align_batch.
//   place_recognition::ScanContextParams    rings x sectors of the polar height image, its range, the sensor's height
//   place_recognition::ScanContext          compute(queue, cloud, params): the descriptor on the device (sp_scan_context_compute)
//   place_recognition::ScanContextDatabase  add(cloud | descriptor), size(), clear(), query(descriptor, k, exclude_recent): every
//                                           entry under every column shift, exactly; the k nearest as LoopCandidates, one read-back
//   place_recognition::initial_guesses      a candidate's yaw as initial guesses for Registration::align_batch / best_of
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "features.hpp"

namespace sycl_points {
namespace algorithms {
namespace place_recognition {

struct ScanContextParams {
    uint32_t rings = 20;          // 1 .. SP_SCAN_CONTEXT_MAX_RINGS
    uint32_t sectors = 60;        // even, 4 .. SP_SCAN_CONTEXT_MAX_SECTORS
    float max_range = 80.0f;      // points at or beyond it are skipped
    float sensor_height = 2.0f;   // added to z, so that the ground is not negative
    sp_scan_context_params c_struct() const { return sp_scan_context_params{rings, sectors, max_range, sensor_height}; }
};

/// rings x sectors floats on the device, ring-major: the maximum of z + sensor_height per polar bin, 0 for an empty bin.
struct ScanContextDescriptor {
    shared_vector_ptr<float> values = nullptr;
    ScanContextParams params;
    size_t size() const { return size_t(params.rings) * params.sectors; }
    const float* device_data() const { return values ? values->device_data() : nullptr; }
};

struct ScanContext {
    /// sp_scan_context_compute on `queue`'s stream. Enqueue only.
    static ScanContextDescriptor compute(const sycl_utils::DeviceQueue& queue, const PointCloudShared& cloud,
                                         const ScanContextParams& params = ScanContextParams()) {
        ScanContextDescriptor out;
        out.params = params;
        out.values = std::make_shared<shared_vector<float>>(queue);
        const sp_scan_context_params p = params.c_struct();
        // (parameters out of range are the library's to report: it writes nothing then, so the buffer is sized within the limits)
        const size_t floats = std::min<size_t>(out.size(), size_t(SP_SCAN_CONTEXT_MAX_RINGS) * SP_SCAN_CONTEXT_MAX_SECTORS);
        throw_on_error(sp_scan_context_compute(&p, cloud.size() ? cloud.points_device() : nullptr, cloud.size(),
                                               out.values->device_data_for_write(std::max<size_t>(floats, 1)), queue.stream()));
        return out;
    }
};

/// One row of ScanContextDatabase::query: the query is entry `index` turned by yaw = shift * 2 pi / sectors about z.
struct LoopCandidate {
    int32_t index = -1;
    float distance = 1.0f;  // in [0, 1]
    int32_t shift = 0;
    float yaw = 0.0f;
    uint32_t sectors = 60;
};

class ScanContextDatabase {
public:
    using Ptr = std::shared_ptr<ScanContextDatabase>;
    explicit ScanContextDatabase(const sycl_utils::DeviceQueue& queue, const ScanContextParams& params = ScanContextParams(),
                                 size_t capacity_hint = 0)
        : queue_(queue), params_(params) {
        const sp_scan_context_params p = params.c_struct();
        throw_on_error(sp_scan_context_db_create(&p, capacity_hint, &db_));
    }
    ~ScanContextDatabase() { sp_scan_context_db_destroy(db_); }
    ScanContextDatabase(const ScanContextDatabase&) = delete;
    ScanContextDatabase& operator=(const ScanContextDatabase&) = delete;

    const ScanContextParams& params() const { return params_; }
    size_t size() const { return sp_scan_context_db_size(db_); }
    void clear() { throw_on_error(sp_scan_context_db_clear(db_)); }

    /// Appends the descriptor (enqueue only); returns the new entry's index.
    size_t add(const ScanContextDescriptor& descriptor) {
        check_shape(descriptor);
        throw_on_error(sp_scan_context_db_add(db_, descriptor.device_data(), queue_.stream()));
        return size() - 1;
    }
    size_t add(const PointCloudShared& cloud) { return add(ScanContext::compute(queue_, cloud, params_)); }

    /// The k nearest entries among all but the `exclude_recent` most recent, nearest first (fewer than k when the range holds
    /// fewer). One read-back of 12 k bytes.
    std::vector<LoopCandidate> query(const ScanContextDescriptor& descriptor, size_t k, size_t exclude_recent = 0) {
        std::vector<LoopCandidate> out;
        check_shape(descriptor);
        const size_t n = size(), count = n > exclude_recent ? n - exclude_recent : 0;
        if (count == 0 || k == 0) return out;
        hipStream_t st = queue_.stream();
        detail::DeviceScratch ws(sp_scan_context_db_search_workspace_bytes(db_, count), st), rows(12 * k, st);
        int32_t* idx = static_cast<int32_t*>(rows.p);
        float* dist = reinterpret_cast<float*>(idx + k);
        int32_t* shift = idx + 2 * k;
        throw_on_error(sp_scan_context_db_search(db_, descriptor.device_data(), 0, count, k, idx, dist, shift, ws.p, ws.bytes, st));
        std::vector<int32_t> host(3 * k);
        hip_check(hipMemcpyAsync(host.data(), rows.p, 12 * k, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipStreamSynchronize(st), "sync");
        for (size_t r = 0; r < k && host[r] >= 0; ++r) {
            LoopCandidate c;
            c.index = host[r];
            std::memcpy(&c.distance, &host[k + r], sizeof(float));
            c.shift = host[2 * k + r];
            c.sectors = params_.sectors;
            c.yaw = static_cast<float>(double(c.shift) * (2.0 * M_PI) / double(params_.sectors));
            out.push_back(c);
        }
        return out;
    }
    std::vector<LoopCandidate> query(const PointCloudShared& cloud, size_t k, size_t exclude_recent = 0) {
        return query(ScanContext::compute(queue_, cloud, params_), k, exclude_recent);
    }

private:
    void check_shape(const ScanContextDescriptor& d) const {
        if (!d.values || d.params.rings != params_.rings || d.params.sectors != params_.sectors)
            throw std::invalid_argument("[ScanContextDatabase] the descriptor's rings x sectors are not the database's");
    }
    sycl_utils::DeviceQueue queue_;
    ScanContextParams params_;
    sp_scan_context_db* db_ = nullptr;
};

/// `steps` poses Rz(-(shift + delta) 2 pi / sectors), delta evenly over [-1/2, 1/2] sector (sp_scan_context_guesses_host): they take
/// the query's points into the candidate's frame up to the translation — the initial guesses of Registration::align_batch for
/// aligning the query scan to the candidate's, best_of picks the winner.
inline std::vector<TransformMatrix> initial_guesses(const LoopCandidate& candidate, size_t steps) {
    ScanContextParams params;
    params.sectors = candidate.sectors;
    const sp_scan_context_params p = params.c_struct();
    std::vector<double> poses(16 * steps);
    throw_on_error(sp_scan_context_guesses_host(&p, static_cast<uint32_t>(candidate.shift), steps, poses.data()));
    std::vector<TransformMatrix> guesses(steps);
    for (size_t g = 0; g < steps; ++g)
        for (int i = 0; i < 16; ++i) guesses[g].data()[i] = static_cast<float>(poses[16 * g + i]);
    return guesses;
}

}  // namespace place_recognition
}  // namespace algorithms
}  // namespace sycl_points
