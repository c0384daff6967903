// sycl_points facade for MI355X — algorithms/mapping/voxel_hash_map.hpp:22-250 (VoxelHashMap) over the sp_vhm_* entry
// points. Same public surface as the reference: constructor (queue, voxel_size), the five setters / getters, clear,
// add_point_cloud(cloud, sensor_pose), downsampling(result, center, distance), compute_overlap_ratio, remove_old_data.
// algorithms/mapping/occupancy_grid_map.hpp:27-472 (OccupancyGridMap) over the sp_ogm_* entry points: the reference's public
// signatures.
// The tables live in HBM inside the library objects; clouds go in and come out through their device mirrors.
#pragma once
#include "core.hpp"

namespace sycl_points {
namespace algorithms {
namespace mapping {

namespace detail {

/// The averaged export of either map (sp_vhm_downsampling, sp_ogm_extract_occupied_points, sp_ogm_extract_visible_points: one shape
/// after their own leading arguments, which `call` binds): `result`'s device arrays sized for the map's voxels, written by the entry
/// point, cut to the rows that came out; an attribute the map does not hold is cleared.
/// call(points, covs, rgb, intensities, capacity, &n) -> the entry point's status.
static_assert(+SP_VHM_INFO_VOXEL_NUM == +SP_OGM_INFO_VOXEL_NUM && +SP_VHM_INFO_HAS_COV == +SP_OGM_INFO_HAS_COV &&
              +SP_VHM_INFO_HAS_RGB == +SP_OGM_INFO_HAS_RGB && +SP_VHM_INFO_HAS_INTENSITY == +SP_OGM_INFO_HAS_INTENSITY);
template <class Handle, class Call>
void mean_rows(Call&& call, size_t (*info)(const Handle*, int), const Handle* h, PointCloudShared& result) {
    const size_t cap = info(h, SP_VHM_INFO_VOXEL_NUM);
    if (cap == 0) { result.clear(); return; }
    const bool has_cov = info(h, SP_VHM_INFO_HAS_COV), has_rgb = info(h, SP_VHM_INFO_HAS_RGB), has_int = info(h, SP_VHM_INFO_HAS_INTENSITY);
    size_t n = 0;
    throw_on_error(call(reinterpret_cast<float*>(result.points->device_data_for_write(cap)),
                        has_cov ? reinterpret_cast<float*>(result.covs->device_data_for_write(cap)) : nullptr,
                        has_rgb ? reinterpret_cast<float*>(result.rgb->device_data_for_write(cap)) : nullptr,
                        has_int ? result.intensities->device_data_for_write(cap) : nullptr, cap, &n));
    result.points->set_device_size(n);
    if (has_cov) result.covs->set_device_size(n); else result.covs->clear();
    if (has_rgb) result.rgb->set_device_size(n); else result.rgb->clear();
    if (has_int) result.intensities->set_device_size(n); else result.intensities->clear();
    result.normals->clear();
    result.timestamp_offsets->clear();
}

/// compute_overlap_ratio of either map over its sp_*_overlap_ratio entry point
template <class Handle>
float overlap_ratio(int (*entry_point)(const Handle*, const float*, size_t, const float*, float*, void*), const Handle* h,
                    const PointCloudShared& cloud, const Eigen::Isometry3f& sensor_pose, void* stream) {
    if (!cloud.points || cloud.points->empty()) return 0.0f;
    float r = 0.0f;
    throw_on_error(entry_point(h, cloud.points_device(), cloud.size(), sensor_pose.matrix().data(), &r, stream));
    return r;
}

}  // namespace detail

class VoxelHashMap {
public:
    using Ptr = std::shared_ptr<VoxelHashMap>;

    VoxelHashMap(const sycl_utils::DeviceQueue& queue, const float voxel_size) : queue_(queue) {
        throw_on_error(sp_vhm_create(voxel_size, queue_.stream(), &h_));  // voxel_size <= 0: std::invalid_argument
    }
    ~VoxelHashMap() { sp_vhm_destroy(h_); }
    VoxelHashMap(const VoxelHashMap&) = delete;
    VoxelHashMap& operator=(const VoxelHashMap&) = delete;

    void set_voxel_size(const float voxel_size) { throw_on_error(sp_vhm_set(h_, SP_VHM_VOXEL_SIZE, voxel_size)); }
    float get_voxel_size() const { return sp_vhm_get(h_, SP_VHM_VOXEL_SIZE); }
    void set_max_staleness(const uint32_t v) { throw_on_error(sp_vhm_set(h_, SP_VHM_MAX_STALENESS, (float)v)); }
    uint32_t get_max_staleness() const { return (uint32_t)sp_vhm_get(h_, SP_VHM_MAX_STALENESS); }
    void set_remove_old_data_cycle(const uint32_t v) { throw_on_error(sp_vhm_set(h_, SP_VHM_REMOVE_OLD_DATA_CYCLE, (float)v)); }
    uint32_t get_remove_old_data_cycle() const { return (uint32_t)sp_vhm_get(h_, SP_VHM_REMOVE_OLD_DATA_CYCLE); }
    void set_rehash_threshold(const float v) { throw_on_error(sp_vhm_set(h_, SP_VHM_REHASH_THRESHOLD, v)); }
    float get_rehash_threshold() const { return sp_vhm_get(h_, SP_VHM_REHASH_THRESHOLD); }
    void set_min_num_point(const uint32_t v) { throw_on_error(sp_vhm_set(h_, SP_VHM_MIN_NUM_POINT, (float)v)); }
    uint32_t get_min_num_point() const { return (uint32_t)sp_vhm_get(h_, SP_VHM_MIN_NUM_POINT); }

    /// voxel_hash_map.hpp:83-113
    void clear() { throw_on_error(sp_vhm_clear(h_, queue_.stream())); }

    /// voxel_hash_map.hpp:117-141 — cloud in the sensor frame, sensor_pose in the map frame.
    void add_point_cloud(const PointCloudShared& cloud, const Eigen::Isometry3f& sensor_pose) {
        const size_t N = cloud.size();
        throw_on_error(sp_vhm_add_point_cloud(
            h_, N ? cloud.points_device() : nullptr, N ? cloud.covs_device() : nullptr,
            (N && cloud.has_rgb()) ? reinterpret_cast<const float*>(cloud.rgb->device_data()) : nullptr,
            (N && cloud.has_intensity()) ? cloud.intensities->device_data() : nullptr, N, sensor_pose.matrix().data(),
            queue_.stream()));
    }

    /// voxel_hash_map.hpp:146-190 — voxel means whose centroid lies in the box center +- distance.
    void downsampling(PointCloudShared& result, const Eigen::Vector3f& center, const float distance = 100.0f) {
        const float c[3] = {center.x(), center.y(), center.z()};
        detail::mean_rows([&](float* p, float* cv, float* rgb, float* in, size_t cap, size_t* n) {
            return sp_vhm_downsampling(h_, c, distance, p, cv, rgb, in, nullptr, cap, n, queue_.stream());
        }, sp_vhm_info, h_, result);
    }

    /// voxel_hash_map.hpp:196-246
    float compute_overlap_ratio(const PointCloudShared& cloud, const Eigen::Isometry3f& sensor_pose) const {
        return detail::overlap_ratio(sp_vhm_overlap_ratio, h_, cloud, sensor_pose, queue_.stream());
    }

    void remove_old_data() { throw_on_error(sp_vhm_remove_old_data(h_, queue_.stream())); }

    /// MI355X extension: the rows Registration::align(source, map) reads (sp_vhm_prepare_registration), for the map as it is
    /// now; reg_type SP_REG_GICP or SP_REG_POINT_TO_DISTRIBUTION. align() calls it when registration_ready() says no.
    void prepare_registration(const int reg_type) { throw_on_error(sp_vhm_prepare_registration(h_, reg_type, queue_.stream())); }
    bool registration_ready(const int reg_type) const { return sp_vhm_registration_ready(h_, reg_type) != 0; }
    const sp_voxel_hash_map* handle() const { return h_; }

private:
    sycl_utils::DeviceQueue queue_;
    sp_voxel_hash_map* h_ = nullptr;
};

class OccupancyGridMap {
public:
    using Ptr = std::shared_ptr<OccupancyGridMap>;

    OccupancyGridMap(const sycl_utils::DeviceQueue& queue, const float voxel_size) : queue_(queue) {
        throw_on_error(sp_ogm_create(voxel_size, queue_.stream(), &h_));  // voxel_size <= 0: std::invalid_argument
    }
    ~OccupancyGridMap() { sp_ogm_destroy(h_); }
    OccupancyGridMap(const OccupancyGridMap&) = delete;
    OccupancyGridMap& operator=(const OccupancyGridMap&) = delete;

    /// occupancy_grid_map.hpp:42-69
    void clear() { throw_on_error(sp_ogm_clear(h_, queue_.stream())); }

    void set_voxel_size(const float voxel_size) { throw_on_error(sp_ogm_set(h_, SP_OGM_VOXEL_SIZE, voxel_size)); }
    float voxel_size() const { return sp_ogm_get(h_, SP_OGM_VOXEL_SIZE); }

    /// occupancy_grid_map.hpp:85-93 — 0.5 where the map holds no voxel
    float voxel_probability(const Eigen::Vector3f& position) const {
        const float p[3] = {position.x(), position.y(), position.z()};
        float r = 0.5f;
        throw_on_error(sp_ogm_voxel_probability(h_, p, &r, queue_.stream()));
        return r;
    }

    void set_log_odds_hit(const float value) { throw_on_error(sp_ogm_set(h_, SP_OGM_LOG_ODDS_HIT, value)); }
    void set_log_odds_miss(const float value) { throw_on_error(sp_ogm_set(h_, SP_OGM_LOG_ODDS_MISS, value)); }
    void set_free_space_updates_enabled(const bool enabled) {
        throw_on_error(sp_ogm_set(h_, SP_OGM_FREE_SPACE_UPDATES, enabled ? 1.0f : 0.0f));
    }
    void set_voxel_pruning_enabled(const bool enabled) { throw_on_error(sp_ogm_set(h_, SP_OGM_VOXEL_PRUNING, enabled ? 1.0f : 0.0f)); }
    void set_log_odds_limits(const float minimum, const float maximum) {  // minimum > maximum: std::invalid_argument
        throw_on_error(sp_ogm_set_log_odds_limits(h_, minimum, maximum));
    }
    void set_occupancy_threshold(const float probability) {  // outside (0, 1): std::invalid_argument
        throw_on_error(sp_ogm_set(h_, SP_OGM_OCCUPANCY_THRESHOLD, probability));
    }
    void set_stale_frame_threshold(const uint32_t threshold) {
        throw_on_error(sp_ogm_set(h_, SP_OGM_STALE_FRAME_THRESHOLD, (float)threshold));
    }

    /// occupancy_grid_map.hpp:129-163 — cloud in the sensor frame, sensor_pose in the map frame.
    void add_point_cloud(const PointCloudShared& cloud, const Eigen::Isometry3f& sensor_pose) {
        if (!cloud.points || cloud.points->empty()) return;
        const size_t N = cloud.size();
        throw_on_error(sp_ogm_add_point_cloud(
            h_, cloud.points_device(), cloud.covs_device(),
            cloud.has_rgb() ? reinterpret_cast<const float*>(cloud.rgb->device_data()) : nullptr,
            cloud.has_intensity() ? cloud.intensities->device_data() : nullptr, N, sensor_pose.matrix().data(), queue_.stream()));
    }

    /// occupancy_grid_map.hpp:169-181 — occupied voxels within max_distance (L-infinity) of the sensor, in table-slot order.
    void extract_occupied_points(PointCloudShared& result, const Eigen::Isometry3f& sensor_pose,
                                 const float max_distance = 100.0f) const {
        const Eigen::Vector3f t = sensor_pose.translation();
        const float c[3] = {t.x(), t.y(), t.z()};
        detail::mean_rows([&](float* p, float* cv, float* rgb, float* in, size_t cap, size_t* n) {
            return sp_ogm_extract_occupied_points(h_, c, max_distance, p, cv, rgb, in, nullptr, cap, n, queue_.stream());
        }, sp_ogm_info, h_, result);
    }

    /// occupancy_grid_map.hpp:183-411 — of those, the voxels within max_distance (L2) inside the frustum of the two fields of view
    /// (radians, around the sensor's x axis) that no other occupied voxel hides; in table-slot order. On an empty map every
    /// attribute of `result` is resized to 0 (the reference resizes points and covariances only).
    void extract_visible_points(PointCloudShared& result, const Eigen::Isometry3f& sensor_pose, float max_distance,
                                float horizontal_fov, float vertical_fov) const {
        detail::mean_rows([&](float* p, float* cv, float* rgb, float* in, size_t cap, size_t* n) {
            return sp_ogm_extract_visible_points(h_, sensor_pose.matrix().data(), max_distance, horizontal_fov, vertical_fov, p, cv,
                                                 rgb, in, nullptr, cap, n, queue_.stream());
        }, sp_ogm_info, h_, result);
    }

    /// occupancy_grid_map.hpp:417-472
    float compute_overlap_ratio(const PointCloudShared& cloud, const Eigen::Isometry3f& sensor_pose) const {
        return detail::overlap_ratio(sp_ogm_overlap_ratio, h_, cloud, sensor_pose, queue_.stream());
    }

private:
    sycl_utils::DeviceQueue queue_;
    sp_occupancy_grid_map* h_ = nullptr;
};

}  // namespace mapping
}  // namespace algorithms
}  // namespace sycl_points
