// VoxelHashMap for gfx950 — submap accumulation either side of the hot path (replaces
// algorithms/mapping/voxel_hash_map.hpp:22-1072).
//
// The table is sp_voxel_table.h's with a 16-byte core {sum xyz, count} and 100 probes; the host state, the compaction scratch and
// the overlap kernel are there too. One lane per input point: transform into the map frame (the reference's fma chain),
// compute_voxel_bit (the K9 key), rotate + log-map the covariance, claim or find the slot with a 64-bit compare-and-swap and add with relaxed
// device-scope atomics (global_atomic_add_f32 executes at the memory side on gfx950; ~1.3 TB/s of added bytes chip-wide,
// MI355X_MICROARCH.md "Global float atomics"). The reference pre-reduces inside a work-group with a bitonic sort before its
// atomics; here that step is dropped: 60 B of atomics per point at 1M points is ~50 us, less than the sort.
// As in the reference the accumulation order is unspecified (float sums agree to rounding, counts exactly).
// Export (downsampling) is deterministic: slot order via flags + exclusive scan (the reference's NVIDIA path, :947-985).
// Host-side control flow (rehash schedule, staleness counter, has_* flags) follows :117-141 line by line; like the
// reference, add_point_cloud waits for its kernel and reads the voxel count back.

#include "voxel_hash_map.h"

namespace sp {
namespace {

constexpr unsigned kMaxProbe = kVhmMaxProbe;

using Table = VhmTable;

// global_reduction (:549-585): claim the first free slot or find the key's slot within kMaxProbe probes, then add.
// An entry that finds neither is dropped, as in the reference.
// Not OccupancyGridMap's find_or_claim, on purpose: this one swaps first, probes 100 times and knows no `deleted` key.
__device__ __forceinline__ void insert(const Table& t, uint64_t h, float sx, float sy, float sz, unsigned count,
                                       const CovSum& cv, bool has_cov, const float4 col, bool has_rgb, float inten,
                                       bool has_intensity, uint32_t when, unsigned* __restrict__ voxel_num) {
    if (h == kInvalidKey) return;
    for (unsigned p = 0; p < kMaxProbe; ++p) {
        const unsigned long long s = slot_id(h, p, t.capacity);
        const unsigned long long seen = atomicCAS(reinterpret_cast<unsigned long long*>(t.key + s), kInvalidKey, h);
        if (seen == kInvalidKey) atomicAdd(voxel_num, 1u);
        else if (seen != h) continue;
        float* core = reinterpret_cast<float*>(t.core + s);
        fadd(core + 0, sx);
        fadd(core + 1, sy);
        fadd(core + 2, sz);
        atomicAdd(reinterpret_cast<unsigned*>(core + 3), count);
        add_attributes(t, s, cv, has_cov, col, has_rgb, inten, has_intensity);
        stamp(t, s, when);  // :325-328
        return;
    }
}

// add_point_cloud_impl (:594-786): load_entry + global_reduction, one lane per point
__global__ __launch_bounds__(kBlock) void vhm_add_kernel(Table t, const float4* __restrict__ pts,
                                                         const float4* __restrict__ covs, const float4* __restrict__ rgb,
                                                         const float* __restrict__ inten, unsigned n, Mat4Arg pose,
                                                         float inv, bool map_has_cov, bool map_has_rgb,
                                                         bool map_has_intensity, uint32_t stamp,
                                                         unsigned* __restrict__ voxel_num) {
    const Rigid T = load_rigid_colmajor(pose.m);
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float4 p = pts[i];
        float wx, wy, wz;
        transform_point(T, p.x, p.y, p.z, wx, wy, wz);
        const uint64_t h = voxel_key3(wx, wy, wz, inv);
        CovSum cv{0, 0, 0, 0, 0, 0};
        if (covs && h != kInvalidKey) cv = encode_cov(covs + 4 * (size_t)i, T);  // (:460-480)
        const float4 col = rgb ? rgb[i] : make_float4(0, 0, 0, 0);
        insert(t, h, wx, wy, wz, 1u, cv, map_has_cov, col, map_has_rgb, inten ? inten[i] : 0.0f, map_has_intensity, stamp,
               voxel_num);
    }
}

// rehash (:845-931): every live slot of the old table re-enters the new one with its own time stamp.
// Not OccupancyGridMap's rehash kernel, on purpose: a table whose probe chains vhm_remove_kernel has cut can hold one key twice (the
// next insert of a key that sits behind a slot reset to `invalid` claims that slot, short of its own), and re-entering through
// insert() merges the two entries with its atomic adds.
__global__ __launch_bounds__(kBlock) void vhm_rehash_kernel(Table old_t, Table new_t, bool has_cov, bool has_rgb,
                                                            bool has_intensity, unsigned* __restrict__ voxel_num) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= old_t.capacity) return;
    const uint64_t k = old_t.key[i];
    if (k == kInvalidKey) return;
    const float4 c = old_t.core[i];
    insert(new_t, k, c.x, c.y, c.z, __float_as_uint(c.w), has_cov ? old_t.cov[i] : CovSum{0, 0, 0, 0, 0, 0}, has_cov,
           has_rgb ? old_t.color[i] : make_float4(0, 0, 0, 0), has_rgb, has_intensity ? old_t.intensity[i] : 0.0f,
           has_intensity, old_t.last_update[i], voxel_num);
}

// remove_old_data_impl (:788-843)
__global__ __launch_bounds__(kBlock) void vhm_remove_kernel(Table t, uint32_t remove_staleness,
                                                            unsigned* __restrict__ voxel_num) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity) return;
    if (t.key[i] == kInvalidKey) return;
    if (t.last_update[i] >= remove_staleness) { atomicAdd(voxel_num, 1u); return; }
    t.key[i] = kInvalidKey;
    t.core[i] = make_float4(0, 0, 0, 0);
    t.cov[i] = CovSum{0, 0, 0, 0, 0, 0};
    t.color[i] = make_float4(0, 0, 0, 0);
    t.intensity[i] = 0.0f;
    t.last_update[i] = 0;
}

// should_include_voxel (:402-418). Each map's flag kernel tests its own condition: not shared.
__global__ __launch_bounds__(kBlock) void vhm_flag_kernel(Table t, uint32_t min_num_point, float mnx, float mny, float mnz,
                                                          float mxx, float mxy, float mxz, unsigned* __restrict__ flags) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity) return;
    const float4 c = t.core[i];
    const unsigned count = __float_as_uint(c.w);
    bool keep = t.key[i] != kInvalidKey && count >= min_num_point && count != 0u;
    if (keep) {
        const float inv = 1.0f / (float)count;
        const float cx = c.x * inv, cy = c.y * inv, cz = c.z * inv;
        keep = (cx >= mnx && cx <= mxx) && (cy >= mny && cy <= mxy) && (cz >= mnz && cz <= mxz);
    }
    flags[i] = keep ? 1u : 0u;
}

// compute_averaged_attributes (:330-386) into the compacted outputs (slot order)
__global__ __launch_bounds__(kBlock) void vhm_export_kernel(Table t, const unsigned* __restrict__ flags,
                                                            const unsigned* __restrict__ pos, unsigned out_capacity, MeanRows out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= t.capacity || !flags[i]) return;
    const unsigned o = pos[i];
    if (o >= out_capacity) return;
    const float4 c = t.core[i];
    write_mean_row(t, i, o, __float_as_uint(c.w), c.x, c.y, c.z, out);
}

// compute_overlap_ratio (:196-246): a voxel counts from min_num_point points on
struct EnoughPoints {
    uint32_t min_num_point;
    __device__ bool operator()(const float4& core) const { return __float_as_uint(core.w) >= min_num_point; }
};

}  // namespace
}  // namespace sp

namespace sp {
namespace {

void drop_flags_when_empty(sp_voxel_hash_map* m) {  // update_voxel_num_and_flags (:519-526), after a count was read back
    if (m->voxel_num == 0) m->has_cov = m->has_rgb = m->has_intensity = false;
}

auto rehash_launch(const sp_voxel_hash_map* m, hipStream_t st) {
    return [=](const Table& old_t, const Table& new_t) {
        vhm_rehash_kernel<<<div_up(old_t.capacity, kBlock), kBlock, 0, st>>>(old_t, new_t, m->has_cov, m->has_rgb, m->has_intensity,
                                                                            m->counter);
    };
}

int remove_old(sp_voxel_hash_map* m, hipStream_t st) {
    if (m->staleness_counter <= m->max_staleness) return SP_OK;
    int rc = m->write_counter(st, 0);
    if (rc != SP_OK) return rc;
    m->touch();
    vhm_remove_kernel<<<div_up(m->t.capacity, kBlock), kBlock, 0, st>>>(m->t, m->staleness_counter - m->max_staleness,
                                                                      m->counter);
    if ((rc = m->read_voxel_num(st)) == SP_OK) drop_flags_when_empty(m);
    return rc;
}

}  // namespace
}  // namespace sp

extern "C" int sp_vhm_create(float voxel_size, void* stream, sp_voxel_hash_map** out) {
    return sp::create_map(voxel_size, stream, out);
}
extern "C" void sp_vhm_destroy(sp_voxel_hash_map* m) {
    if (m) (void)hipFree(m->reg_rows);
    sp::destroy_map(m);
}

extern "C" int sp_vhm_clear(sp_voxel_hash_map* m, void* stream) {  // :83-113
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    m->touch();
    const int rc = m->reset_to_first_capacity(sp::as_stream(stream));
    if (rc == SP_OK) m->staleness_counter = 0;
    return rc;
}

extern "C" int sp_vhm_set(sp_voxel_hash_map* m, int param, float value) {
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    switch (param) {
        case SP_VHM_VOXEL_SIZE:
            if (!(value > 0.0f)) { sp_set_error("voxel_size must be positive."); return SP_ERR_INVALID_ARGUMENT; }
            m->voxel_size = value;
            m->voxel_size_inv = 1.0f / value;
            m->touch();
            return SP_OK;
        case SP_VHM_MAX_STALENESS: m->max_staleness = (uint32_t)value; return SP_OK;
        case SP_VHM_REMOVE_OLD_DATA_CYCLE: m->remove_old_data_cycle = (uint32_t)value; return SP_OK;
        case SP_VHM_REHASH_THRESHOLD: m->rehash_threshold = value; return SP_OK;
        case SP_VHM_MIN_NUM_POINT: m->min_num_point = (uint32_t)value; m->touch(); return SP_OK;
    }
    return SP_ERR_INVALID_ARGUMENT;
}
extern "C" float sp_vhm_get(const sp_voxel_hash_map* m, int param) {
    if (!m) return 0.0f;
    switch (param) {
        case SP_VHM_VOXEL_SIZE: return m->voxel_size;
        case SP_VHM_MAX_STALENESS: return (float)m->max_staleness;
        case SP_VHM_REMOVE_OLD_DATA_CYCLE: return (float)m->remove_old_data_cycle;
        case SP_VHM_REHASH_THRESHOLD: return m->rehash_threshold;
        case SP_VHM_MIN_NUM_POINT: return (float)m->min_num_point;
    }
    return 0.0f;
}
extern "C" size_t sp_vhm_info(const sp_voxel_hash_map* m, int what) {
    if (!m) return 0;
    switch (what) {
        case SP_VHM_INFO_VOXEL_NUM: return m->voxel_num;
        case SP_VHM_INFO_CAPACITY: return (size_t)m->t.capacity;
        case SP_VHM_INFO_STALENESS_COUNTER: return m->staleness_counter;
        case SP_VHM_INFO_HAS_COV: return m->has_cov;
        case SP_VHM_INFO_HAS_RGB: return m->has_rgb;
        case SP_VHM_INFO_HAS_INTENSITY: return m->has_intensity;
    }
    return 0;
}

extern "C" int sp_vhm_remove_old_data(sp_voxel_hash_map* m, void* stream) {
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    return sp::remove_old(m, sp::as_stream(stream));
}

// add_point_cloud (:117-141)
extern "C" int sp_vhm_add_point_cloud(sp_voxel_hash_map* m, const float* points, const float* covs, const float* rgb,
                                      const float* intensities, size_t n, const float* sensor_pose_host16, void* stream) {
    using namespace sp;
    if (!m || (n && !points)) return SP_ERR_INVALID_ARGUMENT;
    if (n >= (1ull << 32)) { sp_set_error("[VoxelHashMap] more than 2^32 points"); return SP_ERR_INVALID_ARGUMENT; }
    hipStream_t st = as_stream(stream);
    const unsigned long long cap = m->t.capacity;
    m->touch();  // (before anything is enqueued: a call that fails half way leaves rows nobody may trust either)
    int rc = m->ensure_rehash(st, rehash_launch(m, st));
    if (rc != SP_OK) return rc;
    if (m->t.capacity != cap) drop_flags_when_empty(m);
    // Unlike OccupancyGridMap, an empty cloud still is a frame: the staleness counter advances and the removal pass may run.
    if (n > 0) {
        m->note_attributes(covs, rgb, intensities);
        if ((rc = m->write_counter(st, (unsigned)m->voxel_num)) != SP_OK) return rc;
        vhm_add_kernel<<<stream_grid(n), kBlock, 0, st>>>(
            m->t, reinterpret_cast<const float4*>(points), reinterpret_cast<const float4*>(covs),
            reinterpret_cast<const float4*>(rgb), intensities, (unsigned)n, pose_arg(sensor_pose_host16), m->voxel_size_inv,
            m->has_cov, m->has_rgb, m->has_intensity, m->staleness_counter, m->counter);
        if ((rc = m->read_voxel_num(st)) != SP_OK) return rc;
    }
    if (m->remove_old_data_cycle > 0 && (m->staleness_counter % m->remove_old_data_cycle) == 0)
        if ((rc = remove_old(m, st)) != SP_OK) return rc;
    ++m->staleness_counter;
    return SP_OK;
}

// downsampling (:146-190) + downsampling_impl (:933-1068)
extern "C" int sp_vhm_downsampling(sp_voxel_hash_map* m, const float* center_host3, float distance, float* points_out,
                                   float* covs_out, float* rgb_out, float* intensities_out, uint64_t* keys_out_opt,
                                   size_t out_capacity, size_t* n_out_host, void* stream) {
    using namespace sp;
    if (!m || !center_host3 || !n_out_host) return SP_ERR_INVALID_ARGUMENT;
    *n_out_host = 0;
    if (m->voxel_num == 0) return SP_OK;
    if (!points_out || out_capacity < m->voxel_num) {
        sp_set_error("[VoxelHashMap::downsampling] output arrays must hold sp_vhm_info(SP_VHM_INFO_VOXEL_NUM) entries");
        return SP_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = as_stream(stream);
    int rc = m->ensure_scratch();
    if (rc != SP_OK) return rc;
    const unsigned blocks = div_up((size_t)m->t.capacity, kBlock);
    vhm_flag_kernel<<<blocks, kBlock, 0, st>>>(m->t, m->min_num_point, center_host3[0] - distance, center_host3[1] - distance,
                                               center_host3[2] - distance, center_host3[0] + distance, center_host3[1] + distance,
                                               center_host3[2] + distance, m->flags);
    if ((rc = m->scan_flags(st)) != SP_OK) return rc;
    vhm_export_kernel<<<blocks, kBlock, 0, st>>>(m->t, m->flags, m->pos, (unsigned)out_capacity,
                                                 m->mean_rows(points_out, covs_out, rgb_out, intensities_out, keys_out_opt));
    return m->read_total(st, n_out_host);
}

extern "C" int sp_vhm_overlap_ratio(const sp_voxel_hash_map* m, const float* points, size_t n,
                                    const float* sensor_pose_host16, float* ratio_out_host, void* stream) {
    if (!m) return SP_ERR_INVALID_ARGUMENT;
    return m->overlap_ratio<sp::kMaxProbe>(sp::EnoughPoints{m->min_num_point}, points, n, sensor_pose_host16, ratio_out_host,
                                           sp::as_stream(stream));
}
